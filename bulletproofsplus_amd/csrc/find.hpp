// find.hpp -- verifying a block of containers AND listing the outputs of many view keys in one call: by rewinding its
// single-output proofs (bpp_range_verify_find_serialized_mixed_keys*), the same with one-byte view tags
// (bpp_range_verify_find_tagged_serialized_mixed_keys*), and -- the class step and its kernels in outputs.hpp -- per OUTPUT
// by derived masks (bpp_range_verify_find_outputs_serialized_mixed_keys*); also sealing amounts (bpp_amounts_seal*) and
// making the tags (bpp_view_tags*).  What a scanning service does with a block otherwise is two calls that share a front --
// bpp_range_verify_batch_serialized_mixed_device, then bpp_range_scan_serialized_mixed_keys_device -- and a walk over the
// scan's dense pair matrix; here the front (index upload, decode, membership test, challenges) runs once, the verdict gates
// the confirmation, and the answer is the verdicts and a short ordered list of hits.  The untagged call pays 2k + 3 slot
// expansions, as many products in Fr and a table walk for EVERY (key, single output) pair; in the tagged call a pair first
// pays one SHA-256 compression -- view_tag(key, idx) against the byte the output carries -- and only the pairs that match,
// the CANDIDATES, go on.  Verdicts, hit records, their order and the max_hits rule are the same in all three.  One engine
// (FindEngine: the schedule, the workspace, the host twin) under three MODES of its arguments; what a mode does with a class
// is its CLASS STEP, and a translation unit instantiates the engine with the step whose kernels it owns: RewindStep here
// (tu_find_*.hip: both rewinding modes), OutputStep in outputs.hpp (tu_outputs_*.hip).  find_terms.hpp has the pad, the tag
// and the index arithmetic; what a pair's lanes compute (its Gamma, its confirmation) is recover_keys.hpp's.
//
// A key is paired with the UNITS of the block: its caller positions when proofs are rewound, its caller output numbers
// (the sum of m_i) per output.  The pair region lies key-major, [key][unit].
// Schedule, all on the caller's stream, no host synchronisation beyond the front's index upload (per output its free word
// carries each proof's first caller output number): decode_front; the pair words zeroed where no kernel below will write
// them (untagged: those of aggregated proofs, so only when there are any; tagged: every non-candidate's, so always; per
// output: every pair that does not become a hit, so whenever there are keys); per class present derive_challenges and
// today's exact pass (VerifyImpl::run) into front.ok, then the mode's class step; k_mixed_status_scatter writes d_ok;
// k_find_count, k_find_offsets, k_find_emit make the hit list.  A call without keys -- or, rewinding, without a
// single-output proof -- takes no class step and lists nothing: verdicts, and zero counts.
// The rewinding class steps take the single-output class alone: RecoverKeysImpl's bind_class and launch_coeffs
// (k_recover_coeffs) with Gamma and the pair word pointed at the pair region of the workspace, then
// untagged: k_scan_keys, then
// k_find_confirm: one lane per (key, single-output proof) pair, numbered as k_scan_keys numbers them.  A lane whose proof
// the pass did not accept, the decoder rejected or whose coefficients are undefined clears its pair (no hit, Gamma zero)
// before it reads a key or a Gamma.  Otherwise the candidate amount (find_pair_amount) -- sealed mode: the key's words into
// registers, the pad by amount_pad, amount = sealed XOR pad; else a load from the key-major array -- then pair_confirms.  A
// hit keeps its Gamma and stores its amount; a miss has its Gamma zeroed.
// tagged: the candidate list (launch_candidates, which the per-output step uses too) --
// k_find_tags: one 64-lane block per tile of FIND_TILE launch positions OF ONE KEY (find_terms.hpp), a lane per pair and
// round (tag_tile: the tiling, the ballots and the count, around the kernel's candidate predicate).  A lane whose proof the
// pass did not accept, the decoder rejected or whose coefficients are undefined is no candidate before it reads a key.  The
// others read the tile's key (uniform over the block: scalar loads), the index and the tag byte of their caller position,
// and compress once.  The tile leaves its FIND_ROUNDS ballots and its count: ONE BIT per pair instead of a flag word.
// k_find_offsets scans the tile counts and leaves the candidate count in a workspace word.
// k_find_list: the lanes of the tag kernel again, from the ballots: candidate number h of the class, in ascending key-major
// pair number, to list[h].  No atomics; the same list from run to run.  Where it is given a place it copies the count there:
// the tagged call's n_candidates, its one class.
// -- then k_find_scan_list: k_scan_keys's eight lanes per pair (pair_gamma), over the list: group g takes candidates g,
// g + groups, .. below the count it READS FROM THE WORKSPACE; the grid is sized from n_keys x count alone, so the host never
// learns the count.  Gamma goes to the pair's place in the key-major region.
// k_find_confirm_list: k_find_confirm's lane, one per POSSIBLE pair (the stride over the list is one step: lanes at or
// beyond the count end at once): candidate amount, pair_confirms; a hit sets its pair word and stores its amount, a miss has
// its Gamma zeroed.
// The compaction: the pair words lie key-major ([key][unit]), so ascending position is ascending (key number, caller
// position or output number).  k_find_count: one 64-lane block per tile of FIND_TILE positions, a ballot per round, the
// tile's count.  k_find_offsets: one wave scans the tile counts in place (exclusive) and writes the total to d_n_hits.
// k_find_emit: the lanes of k_find_count again; a hit's place is its tile's offset, the ballots of the rounds before and
// the lanes below it -- no atomics, and an order that does not depend on scheduling.  Records at or beyond max_hits are
// not written.
// The key rule: no LDS, no scratch in any kernel here.  A key's words go from its buffer into registers in one place
// (load_key, recover_keys.hpp).  Nothing derived from a key reaches memory but the candidate bit (the match of a PUBLIC
// byte), the hit bit, Gamma of a pair that was scanned (zeroed on a miss: when the call ends no Gamma of a pair that is not
// a hit is left in the workspace) and a hit's amount.  The Gamma and amount words of non-candidates are never written.
#pragma once
#include "recover_keys.hpp"
#include "find_terms.hpp"
#include "scan_args.hpp"   // FindArgs, FindMode

namespace bpp {

constexpr unsigned FIND_LIST_BLOCKS = 8192;   // most blocks k_find_scan_list is launched with: 32 waves for each of 256 CUs

// one lane per output: out[i] = in[i] XOR pad(key, index of i); in and out may be one buffer.  The key travels by value
// (RecoverSource's reason).
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_amounts_seal(BlindKey key, uint64_t index_base, const uint64_t* __restrict__ index,
                                                             const uint64_t* in, uint64_t* out, size_t count) {
    const size_t i = (size_t)blockIdx.x * FIND_BLOCK + threadIdx.x;
    if (i >= count) return;
    uint32_t kw[8];
    load_key(key.w, 0, kw);
    out[i] = in[i] ^ amount_pad(kw, index ? index[i] : index_base + i);
}

// one lane per output: out[i] = view_tag(key, index of i).  The key travels by value (k_amounts_seal's reason).
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_view_tags(BlindKey key, uint64_t index_base, const uint64_t* __restrict__ index,
                                                          uint8_t* __restrict__ out, size_t count) {
    const size_t i = (size_t)blockIdx.x * FIND_BLOCK + threadIdx.x;
    if (i >= count) return;
    uint32_t kw[8];
    load_key(key.w, 0, kw);
    out[i] = view_tag(kw, index ? index[i] : index_base + i);
}

// what the confirmation kernels take beside the pair job of k_scan_keys (whose out_status is the pair word: 1 for a hit, else 0)
struct FindJob {
    const uint32_t* ok;        // the pass's verdicts, by launch position
    const uint64_t* amounts;   // sealed: count x u64 by caller position; else n_keys x total, key-major
    uint32_t sealed, amount64;
    uint64_t* hit_amounts;     // n_keys x total, key-major; written for hits only
};

// the candidate amount of the pair at place `at` ([key_no][caller]): sealed -- the key's words into registers, the output's
// one ciphertext XOR the key's pad -- else a load from the key-major array
__device__ __forceinline__ uint64_t find_pair_amount(const ScanKeysJob& j, const FindJob& f, size_t key_no, size_t caller,
                                                     size_t at) {
    if (!f.sealed) return f.amounts[at];
    uint32_t key[8];
    const uint64_t idx = pair_key_index(j, key_no, caller, key);
    return f.amounts[caller] ^ amount_pad(key, idx);
}

template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_find_confirm(VerifyShape s, const uint32_t* __restrict__ table, ScanKeysJob j,
                                                             FindJob f, const uint32_t* __restrict__ records, uint32_t nv,
                                                             uint32_t v0) {
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
    const uint64_t amount = find_pair_amount(j, f, key_no, caller, at);
    const bool same = pair_confirms<C>(s, table, j, amount, f.amount64, at, p, records, nv, v0);   // Gamma: k_scan_keys's
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

// what the tagged call keeps beside the untagged call's regions
struct TagJob {
    const uint8_t* tags;    // by caller position
    const uint32_t* ok;     // the pass's verdicts, by launch position
    size_t per_key;         // tiles per key
    uint64_t* ballots;      // tiles x FIND_ROUNDS
    uint32_t* tile_count;   // tiles: counts, then their exclusive scan
    uint32_t* list;         // the candidates' pair numbers (key * count + launch position), ascending
    uint32_t* n_cand;       // one word
};

// Tile blockIdx.x of a tag test, the body of its kernel: per round the lane's launch position, is_candidate(key number,
// position) -- false for a position beyond the class -- the ballot, which lane 0 stores, and the count summed.
template <class Pred>
__device__ __forceinline__ void tag_tile(const TagJob& t, Pred is_candidate) {
    const uint32_t lane = threadIdx.x;
    const size_t tile = blockIdx.x;
    const size_t key_no = tag_tile_key(tile, t.per_key);
    uint32_t n = 0;
#pragma unroll 1
    for (uint32_t r = 0; r < FIND_ROUNDS; r++) {
        const uint64_t ballot = __ballot(is_candidate(key_no, tag_launch_position(tile, t.per_key, r, lane)));
        if (lane == 0) t.ballots[tile * FIND_ROUNDS + r] = ballot;
        n += find_ballot_count(ballot);
    }
    if (lane == 0) t.tile_count[tile] = n;
}

// the tag test of the single-output class; j as k_scan_keys takes it (count: the proofs of the class)
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_find_tags(ScanKeysJob j, TagJob t) {
    tag_tile(t, [&](size_t key_no, size_t p) {
        if (p >= j.count || (t.ok[p] | j.status[p] | j.bad[p])) return false;   // a verified proof with a defined Gamma: only then a key is read
        const size_t caller = j.rx[p * RX_WORDS + RX_CALLER];
        uint32_t key[8];
        const uint64_t idx = pair_key_index(j, key_no, caller, key);
        return view_tag(key, idx) == t.tags[caller];
    });
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
    const size_t groups = (size_t)gridDim.x * (SCAN_BLOCK / SCAN_GROUP);
    const size_t n = n_cand[0];
#pragma unroll 1
    for (size_t c = ((size_t)blockIdx.x * SCAN_BLOCK + threadIdx.x) / SCAN_GROUP; c < n; c += groups) {   // a whole group
        const size_t q = list[c];
        const size_t key_no = q / j.count, p = q - key_no * j.count;
        const size_t caller = j.rx[p * RX_WORDS + RX_CALLER];
        pair_gamma<C>(j, key_no, p, caller, key_no * j.total + caller);
    }
}

// k_find_confirm over the candidates, one lane each.  A candidate is a verified proof with a defined Gamma already.
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_find_confirm_list(VerifyShape s, const uint32_t* __restrict__ table, ScanKeysJob j,
                                                                  FindJob f, const uint32_t* __restrict__ records, uint32_t nv,
                                                                  uint32_t v0, const uint32_t* __restrict__ list,
                                                                  const uint32_t* __restrict__ n_cand) {
    // one lane per POSSIBLE pair, so the stride over the list is a single step: the grid comes from n_keys x count alone and
    // a lane at or beyond the count read here ends at once.  (A loop around this body keeps the shape's scalars live
    // across the walk and costs SGPR spill slots -- a private segment -- on two of the three curves.)
    const size_t c = (size_t)blockIdx.x * FIND_BLOCK + threadIdx.x;
    if (c >= n_cand[0]) return;
    const size_t q = list[c];
    const size_t key_no = q / j.count, p = q - key_no * j.count;
    const size_t caller = j.rx[p * RX_WORDS + RX_CALLER];
    const size_t at = key_no * j.total + caller;
    const uint64_t amount = find_pair_amount(j, f, key_no, caller, at);
    if (pair_confirms<C>(s, table, j, amount, f.amount64, at, p, records, nv, v0)) {   // Gamma: k_find_scan_list's
        j.out_status[at] = 1u;
        f.hit_amounts[at] = amount;
    } else {
        const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        st_words<8>(j.out_masks + at * 8, z);
    }
}

template <class C>
struct FindImpl {
    // mode, a.mode: one of the rewinding two
    static size_t workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, size_t n_keys, FindMode mode);
    static int find(bpp_verifier* v, const FindArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);
    static int find_host(bpp_verifier* v, const FindArgs& a);
    // blind_key: 32 bytes (host); d_index: count x u64 or null; d_in, d_out: count x u64 (may be the same buffer)
    static int seal(const uint8_t* blind_key, uint64_t index_base, const uint64_t* d_index, const uint64_t* d_in, size_t count,
                    uint64_t* d_out, hipStream_t st);
    static int seal_host(const uint8_t* blind_key, uint64_t index_base, const uint64_t* index, const uint64_t* in, size_t count,
                         uint64_t* out);
    // blind_key: 32 bytes (host); d_index: count x u64 or null; d_out: count bytes
    static int tags(const uint8_t* blind_key, uint64_t index_base, const uint64_t* d_index, size_t count, uint8_t* d_out,
                    hipStream_t st);
    static int tags_host(const uint8_t* blind_key, uint64_t index_base, const uint64_t* index, size_t count, uint8_t* out);
};

#ifdef BPP_IMPL_DEFINITIONS
// workspace = front (MixedFront, serialized form) | one class pass's workspace | rewinding only: the single-output class's
// coefficients and zero-challenge flags | the pair region, key-major over ALL units (k_scan_keys addresses it so): Gamma,
// the pair word, the amounts of hits | the compaction's tile counts; with tags only: | the tag test's ballots and tile
// counts | the candidate list, each with room for the largest class that is listed | the candidate count, which like
// them one class leaves to the next: the stream orders them.  A function of (m_of, count, n_keys, mode) alone.
template <class C>
struct FindLayout {
    typename VerifyImpl<C>::MixedFront f;
    size_t run, run_bytes, coeffs, bad, masks, hit, hit_amounts, tiles, ballots, tag_tiles, list, n_cand, total;
    size_t units;   // what each key is paired with
};

// what a class step sees of a call in flight
template <class C>
struct FindCall {
    bpp_verifier* v;
    const FindArgs& a;
    const FindLayout<C>& L;
    uint8_t* ws;
    hipStream_t st;
    uint32_t* W(size_t off) const { return reinterpret_cast<uint32_t*>(ws + off); }
    uint64_t* hit_amounts() const { return reinterpret_cast<uint64_t*>(ws + L.hit_amounts); }
};

// The candidates of one class with `positions` launch positions per key: tag_kernel (tag_tile around its predicate) over
// the tiles, their counts scanned, the list made.  ok: the class's verdicts; n_candidates: where k_find_list copies the
// count, or null.  Returns, in t, what the kernels that walk the list read.
template <class C, class Job>
int launch_candidates(const FindCall<C>& c, void (*tag_kernel)(Job, TagJob), const Job& j, const uint32_t* ok, size_t positions,
                      uint32_t* n_candidates, TagJob& t) {
    t = TagJob{c.a.tags, ok, tag_tiles_per_key(positions), reinterpret_cast<uint64_t*>(c.ws + c.L.ballots), c.W(c.L.tag_tiles),
               c.W(c.L.list), c.W(c.L.n_cand)};
    const size_t tiles = tag_tiles(c.a.n_keys, positions);
    hipLaunchKernelGGL(tag_kernel, dim3((unsigned)tiles), dim3(FIND_BLOCK), 0, c.st, j, t);
    hipLaunchKernelGGL(k_find_offsets<C>, dim3(1), dim3(FIND_BLOCK), 0, c.st, t.tile_count, tiles, t.n_cand);
    hipLaunchKernelGGL(k_find_list<C>, dim3((unsigned)tiles), dim3(FIND_BLOCK), 0, c.st, t, positions, n_candidates);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

// The schedule of the file head, once.  S is the class step and says what differs between the modes it serves:
//   units(p, count)          what each key is paired with
//   widest(p)                the most launch positions per key of a tag test: the room of the candidate list
//   coeff_bytes, flag_bytes  its regions between the pass's workspace and the pair region
//   lists(a, p)              whether the call has a pair to test at all
//   open(v, a, lists, p)     what it refuses, and what it writes into the plan before the index is uploaded
//   zero_pairs(a, p)         whether a listing call's pair words must be zeroed first
//   begin(c), klass(c, cv)   of a listing call: once after the front, and after each class's pass
template <class C, class S>
struct FindEngine {
    using V = VerifyImpl<C>;
    using Layout = FindLayout<C>;
    static Layout layout(const bpp_verifier* v, const MixedPlan& p, size_t count, size_t n_keys, FindMode mode) {
        Layout w = {};
        WsCarver o;
        w.units = S::units(p, count);
        const size_t pairs = n_keys * w.units;
        w.f = V::carve_front(o, p, count, true);
        w.run_bytes = V::class_run_max(v, p, V::pass_bytes);
        w.run = o.take(w.run_bytes);
        w.coeffs = o.take(S::coeff_bytes(v, p));
        w.bad = o.take(S::flag_bytes(p));
        w.masks = o.take(pairs * 32);
        w.hit = o.take(pairs * 4);
        w.hit_amounts = o.take(pairs * 8);
        w.tiles = o.take(find_tiles(pairs) * 4);
        if (mode != FIND_REWIND) {
            const size_t widest = S::widest(p), tiles = tag_tiles(n_keys, widest);
            w.ballots = o.take(tiles * FIND_ROUNDS * 8);
            w.tag_tiles = o.take(tiles * 4);
            w.list = o.take(n_keys * widest * 4);
            w.n_cand = o.take(4);
        }
        w.total = o.total;
        return w;
    }

    static size_t workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, size_t n_keys, FindMode mode,
                                  const uint32_t* outs_of = nullptr) {
        MixedPlan p;
        if (!V::container_shape_ok(v) || mixed_plan_serialized(v->s, m_of, count, max_point_bytes<C>(), false, p, outs_of)) return 0;
        return layout(v, p, count, n_keys, mode).total;
    }

    static int find(bpp_verifier* v, const FindArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
        if (int rc = V::container_args_ok(v, a.version)) return rc;
        const size_t count = a.count;
        MixedPlan p;
        int rc = mixed_plan_serialized(v->s, a.m_of, count, (size_t)container_point_bytes<C>(a.version), true, p, a.outs_of);
        if (rc) return rc;
        const Layout L = layout(v, p, count, a.n_keys, a.mode);
        if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
        const bool lists = S::lists(a, p);
        if ((rc = S::open(v, a, lists, p))) return rc;
        const FindCall<C> c{v, a, L, static_cast<uint8_t*>(d_workspace), st};
        const size_t pairs = a.n_keys * L.units;
        rc = V::decode_front(p, L.f, count, a.proofs, a.commitments, a.version, c.ws, st);
        if (rc) return rc;
        // the pair words no kernel below writes (nor their Gamma and amount words, which nothing reads)
        if (lists && S::zero_pairs(a, p)) HIPCHK(zero_words_async(c.W(L.hit), pairs * 4, st));
        S step;
        if (lists && (rc = step.begin(c))) return rc;
        rc = V::for_each_class(v, p, L.f, c.ws, [&](const typename V::ClassView& cv) {
            int rc1 = V::derive_challenges(v, cv.ps, cv.pts, cv.count, cv.challenges, st);
            if (rc1) return rc1;
            rc1 = V::run(v, cv.ps, cv.pts, cv.sc3, cv.count, cv.challenges, c.W(L.f.ok) + cv.first, c.ws + L.run, L.run_bytes,
                         nullptr, nullptr, st);
            return rc1 || !lists ? rc1 : step.klass(c, cv);
        });
        if (rc) return rc;
        if ((rc = V::scatter_verdicts(L.f, c.ws, a.ok, count, st))) return rc;
        if (!lists) {   // verified, and no pair to test or list
            HIPCHK(zero_words_async(a.n_hits, 4, st));
            if (a.tagged() && a.n_candidates) HIPCHK(zero_words_async(a.n_candidates, 4, st));
            return BPP_OK;
        }
        const unsigned tiles = (unsigned)find_tiles(pairs);
        hipLaunchKernelGGL(k_find_count<C>, dim3(tiles), dim3(FIND_BLOCK), 0, st, c.W(L.hit), pairs, c.W(L.tiles));
        hipLaunchKernelGGL(k_find_offsets<C>, dim3(1), dim3(FIND_BLOCK), 0, st, c.W(L.tiles), (size_t)tiles, a.n_hits);
        hipLaunchKernelGGL(k_find_emit<C>, dim3(tiles), dim3(FIND_BLOCK), 0, st, c.W(L.hit), c.hit_amounts(), c.W(L.masks), pairs,
                           L.units, c.W(L.tiles), a.max_hits, a.hits);
        HIPCHK(hipGetLastError());
        return BPP_OK;
    }

    // host buffers in, host verdicts, hit records and counts out: find between copies
    static int find_host(bpp_verifier* v, const FindArgs& a) {
        if (int rc = V::container_args_ok(v, a.version)) return rc;
        MixedPlan p;
        int rc = mixed_plan_serialized(v->s, a.m_of, a.count, (size_t)container_point_bytes<C>(a.version), false, p, a.outs_of);
        if (rc) return rc;
        const size_t units = S::units(p, a.count), pairs = a.n_keys * units;
        DevBuf dk(true);   // the keys: wiped before they are freed, on every way out
        BlockUpload up;
        DevBuf dtg, dok, dhits, dn, dws;
        BPP_TRY(up.upload(p, a.proofs, a.commitments, a.index, a.count, a.amounts, a.sealed ? units : pairs));
        if (a.tagged()) HIPCHK(dtg.upload(a.tags, units));
        HIPCHK(dk.upload(a.keys, a.n_keys * 32));
        const size_t wsb = layout(v, p, a.count, a.n_keys, a.mode).total;
        FindArgs d = a;
        d.proofs = up.proofs.u8();
        d.commitments = up.commitments.u8();
        d.index = up.index.u64();
        d.amounts = up.amounts.u64();
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
        HIPCHK(dn.download(found, a.tagged() ? 8 : 4));
        HIPCHK(dok.download(a.ok, a.count * 4));
        HIPCHK(dhits.download(a.hits, std::min<size_t>(found[0], d.max_hits) * FIND_HIT_WORDS * 4));
        *a.n_hits = found[0];
        if (a.tagged() && a.n_candidates) *a.n_candidates = found[1];
        return BPP_OK;
    }
};

// The class step of the two rewinding modes.  Only single outputs are scanned -- the other classes need not fit a lane
// group -- and their class comes first in gathered order: launch position = gathered position.
template <class C>
struct RewindStep {
    using V = VerifyImpl<C>;
    using K = RecoverKeysImpl<C>;
    static constexpr int CW = coeff_words<typename C::Fr>();
    ScanKeysJob j;

    static size_t units(const MixedPlan&, size_t count) { return count; }
    static size_t widest(const MixedPlan& p) { return p.count[0]; }
    static size_t coeff_bytes(const bpp_verifier* v, const MixedPlan& p) {
        return p.count[0] ? p.count[0] * coeff_elems(V::class_shape(v, 0).s.k) * CW * 4 : 0;
    }
    static size_t flag_bytes(const MixedPlan& p) { return p.count[0] * 4; }
    static bool lists(const FindArgs& a, const MixedPlan& p) { return a.n_keys != 0 && p.count[0] != 0; }
    static int open(const bpp_verifier* v, const FindArgs&, bool lists, MixedPlan&) {
        if (lists && V::class_shape(v, 0).s.k + 2 > RECOVER_GROUP) return fail(BPP_E_ARG, "mask recovery takes shapes with log2(n m) <= 14");
        return BPP_OK;
    }
    // untagged, the pair words of aggregated proofs; tagged, those of every pair that is no candidate
    static bool zero_pairs(const FindArgs& a, const MixedPlan& p) { return a.tagged() || p.count[0] != a.count; }
    int begin(const FindCall<C>& c) {
        j = K::call_job(c.a.keys, c.a.n_keys, c.a.index_base, c.a.index, c.a.count);
        j.out_masks = c.W(c.L.masks);
        j.out_status = c.W(c.L.hit);
        return BPP_OK;
    }
    int klass(const FindCall<C>& c, const typename V::ClassView& cv) {
        if (cv.c != 0) return BPP_OK;
        const FindArgs& a = c.a;
        const FindLayout<C>& L = c.L;
        K::bind_class(cv, c.W(L.f.idx), c.W(L.f.status), c.W(L.bad), c.W(L.coeffs), j);
        BPP_TRY(K::launch_coeffs(cv, c.W(L.coeffs), c.W(L.bad), c.st));
        const FindJob f{c.W(L.f.ok) + cv.first, a.amounts, a.sealed ? 1u : 0u, a.amount64 ? 1u : 0u, c.hit_amounts()};
        const uint32_t* table = c.v->table.u32();
        const uint32_t* records = reinterpret_cast<const uint32_t*>(cv.pts);
        const uint32_t nv = cv.ps.s.NV, v0 = 3 + 2 * cv.ps.s.k;
        const size_t pairs0 = a.n_keys * cv.count;
        if (!a.tagged()) {
            BPP_TRY(K::launch_scan_keys(j, c.st));
            hipLaunchKernelGGL(k_find_confirm<C>, dim3(cdiv(pairs0, FIND_BLOCK)), dim3(FIND_BLOCK), 0, c.st, c.v->s, table, j, f,
                               records, nv, v0);
            HIPCHK(hipGetLastError());
            return BPP_OK;
        }
        TagJob t;
        BPP_TRY(launch_candidates<C>(c, k_find_tags<C>, j, f.ok, cv.count, a.n_candidates, t));
        // the list kernels: grids sized for every pair a candidate, capped; they read the count on the device
        const size_t scan_blocks = std::min<size_t>(cdiv(pairs0 * SCAN_GROUP, SCAN_BLOCK), FIND_LIST_BLOCKS);
        hipLaunchKernelGGL(k_find_scan_list<C>, dim3((unsigned)scan_blocks), dim3(SCAN_BLOCK), 0, c.st, j, t.list, t.n_cand);
        hipLaunchKernelGGL(k_find_confirm_list<C>, dim3(cdiv(pairs0, FIND_BLOCK)), dim3(FIND_BLOCK), 0, c.st, c.v->s, table, j, f,
                           records, nv, v0, t.list, t.n_cand);
        HIPCHK(hipGetLastError());
        return BPP_OK;
    }
};

template <class C>
size_t FindImpl<C>::workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, size_t n_keys, FindMode mode) {
    return FindEngine<C, RewindStep<C>>::workspace_bytes(v, m_of, count, n_keys, mode);
}
template <class C>
int FindImpl<C>::find(bpp_verifier* v, const FindArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
    return FindEngine<C, RewindStep<C>>::find(v, a, d_workspace, workspace_bytes, st);
}
template <class C>
int FindImpl<C>::find_host(bpp_verifier* v, const FindArgs& a) {
    return FindEngine<C, RewindStep<C>>::find_host(v, a);
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
    HIPCHK(dix.upload(index, count * 8));
    HIPCHK(dio.upload(in, count * 8));
    BPP_TRY(seal(blind_key, index_base, dix.u64(), dio.u64(), count, dio.u64(), nullptr));
    HIPCHK(dio.download(out, count * 8));
    return BPP_OK;
}

template <class C>
int FindImpl<C>::tags(const uint8_t* blind_key, uint64_t index_base, const uint64_t* d_index, size_t count, uint8_t* d_out,
                          hipStream_t st) {
    BlindKey key;
    load_key_words(blind_key, key.w);
    hipLaunchKernelGGL(k_view_tags<C>, dim3(cdiv(count, FIND_BLOCK)), dim3(FIND_BLOCK), 0, st, key, index_base, d_index, d_out,
                       count);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int FindImpl<C>::tags_host(const uint8_t* blind_key, uint64_t index_base, const uint64_t* index, size_t count, uint8_t* out) {
    DevBuf dix, dout;
    HIPCHK(dix.upload(index, count * 8));
    HIPCHK(dout.alloc(count));
    BPP_TRY(tags(blind_key, index_base, dix.u64(), count, dout.u8(), nullptr));
    HIPCHK(dout.download(out, count));
    return BPP_OK;
}
#endif  // BPP_IMPL_DEFINITIONS

extern template struct FindImpl<Bls12381>;
extern template struct FindImpl<Secp256k1>;
extern template struct FindImpl<Ed25519>;

}  // namespace bpp
