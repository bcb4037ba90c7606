// recover.hpp -- mask recovery and scanning (bpp_range_recover_masks_mixed*, bpp_range_scan_serialized_mixed*): the
// receiver's side of a range proof.  Whoever holds a proof's blinding scalars -- the blind_key it was made under and its
// index, or the d_blinding buffer -- gets Gamma = gamma_0 + z^2 gamma_1 + .. back out of delta' (recover_terms.hpp has the
// arithmetic and the reference sites) and, for a single output with a candidate amount, learns from V_0 == v g + Gamma h
// whether the output is theirs.  One instantiation per curve (tu_recover_*.hip).
//
// k_recover_masks: a proof is RECOVER_GROUP = 16 lanes, four proofs per wave; lane t holds term t of recover_terms.hpp
// (t < k: round t, two slots; t = k: the final term, two slots; t = k + 1: alpha, one slot), so the slot expansions (two
// SHA-256 compressions each) and the one inversion per term of a proof run side by side, and the lanes of a wave run one
// instruction stream through both.  The terms are summed over the group by a 4-step butterfly of wave_shfl; lane k scales
// the sum and stores it.  No LDS, no atomics, no workspace traffic: nothing derived from the key but Gamma leaves the
// registers.  k + 2 <= 16 for every shape make_shape admits (n, m <= 64: k <= 12); a larger k is BPP_E_ARG.
// k_recover_confirm: one lane per single-output proof with a candidate amount: the lane of k_commit_batch -- the same
// commit_amount_scalar, commit_walk and wire conversion (commit_walk.hpp) -- then the comparison with the decoded V_0.
// (Moving k_commit_batch's body into a device function of its own changed that kernel's SGPR counts, 81 -> 80 and 64 -> 68;
// its code is left as it was and the two kernels share the helpers instead.)
#pragma once
#include "commit.hpp"
#include "recover_terms.hpp"
#include "scan_args.hpp"

namespace bpp {

static_assert(PAIR_BOUND == ONE_LAUNCH && OUTS_LARGEST == 1u << (OUTS_CLASSES - 1), "scan_args.hpp restates these to stay HIP-free");

constexpr unsigned RECOVER_GROUP = 16;   // lanes per proof
constexpr unsigned RECOVER_BLOCK = 64;

// one entry per proof by GATHERED position (built on the host, RX_WORDS 32-bit words): its position in the caller's
// numbering (blinding index, outputs, amounts) and where its blinding scalars and challenge block sit in the caller's
// packed buffers (in scalars).  The words are those the serialized index (mixed.hpp SX_*) leaves free or shares, so a scan
// uploads ONE table: the decoder's, with RX_BLIND filled in (RX_CH belongs to the wire call, SX_PROOF to the decoder).
enum { RX_CH = 0, RX_CALLER = 2, RX_BLIND = 3, RX_WORDS = 4 };
static_assert(RX_CALLER == SX_CALLER && RX_WORDS == SX_WORDS && RX_BLIND != SX_PROOF && RX_BLIND != SX_COMM,
              "the recovery reads the decoder's per-proof index");
// where a launch finds the challenge blocks: one block for all (the literals of the shape), 3 + k scalars per launch
// position (a class region of derived challenges), or through RX_CH (the caller's packed buffer)
enum { RCH_SHARED = 0, RCH_STRIDED, RCH_INDEXED };

// one launch of k_recover_masks: `count` proofs of one shape (n, m), k = log2(n m), entries rx[0 .. count)
struct RecoverJob {
    uint32_t k, m;
    uint64_t lit;   // recover_literals of the shape
    BlindKey key;
    uint32_t have_key;
    uint64_t index_base;
    const uint64_t* index;      // count x u64 by caller position, or null: index_base + caller position
    const uint32_t* blinding;   // the caller's packed 5 + 2 k_i scalars per proof, or null
    const uint32_t* rx;
    const uint32_t* triples;    // [r', s', delta'] per proof, by caller position or by launch position
    uint32_t triples_by_caller;
    const uint32_t* ch;
    uint32_t ch_mode;
    uint32_t* out;              // Gamma, canonical, by caller position or by launch position
    uint32_t out_by_caller;
    uint32_t* conf;             // by launch position, or null: BPP_SCAN_UNCONFIRMED for a zero challenge, else 0
    size_t count;
};

template <class C>
__global__ void __launch_bounds__(RECOVER_BLOCK) k_recover_masks(RecoverJob j) {
    using P = typename C::Fr;
    using F = Fe<P>;
    const uint32_t lane = threadIdx.x & 63u, t = lane & (RECOVER_GROUP - 1);
    const size_t g = ((size_t)blockIdx.x * RECOVER_BLOCK + threadIdx.x) / RECOVER_GROUP;
    const bool live = g < j.count;
    const size_t p = live ? g : j.count - 1;   // an idle group of the last wave repeats the last proof and stores nothing
    const uint32_t* e = j.rx + p * RX_WORDS;
    const size_t caller = e[RX_CALLER];
    RecoverSource src;
    src.have_key = j.have_key != 0;
#pragma unroll
    for (int w = 0; w < 8; w++) src.key[w] = j.key.w[w];
    src.idx = j.index ? j.index[caller] : j.index_base + caller;
    src.blind = j.blinding ? j.blinding + (size_t)e[RX_BLIND] * 8 : nullptr;
    src.lit = j.lit;
    const uint32_t* triple = j.triples + (j.triples_by_caller ? caller : p) * 24;
    const uint32_t* ch = j.ch;
    if (j.ch_mode == RCH_STRIDED) ch += p * (size_t)(3 + j.k) * 8;
    if (j.ch_mode == RCH_INDEXED) ch += (size_t)e[RX_CH] * 8;
    F scale = F::one();
    bool ok;
    F sum = recover_term<P>(src, j.k, j.m, t, triple, ch, scale, ok, [](const F& x) { return fe_inv(x); });
    uint32_t bad = ok ? 0u : 1u;
#pragma unroll 1
    for (int d = RECOVER_GROUP >> 1; d >= 1; d >>= 1) {
        sum = fe_add(sum, wave_shfl(sum, (int)(lane ^ d)));
        bad |= (uint32_t)__shfl((int)bad, (int)(lane ^ d), 64);
    }
    if (live && t == j.k) {
        uint32_t o[8];
        fe_to_canonical(bad ? F::zero() : fe_mul(sum, scale), o);   // a zero challenge: Gamma = 0
        st_words<8>(j.out + (j.out_by_caller ? caller : p) * 8, o);
        if (j.conf) j.conf[p] = bad ? (uint32_t)BPP_SCAN_UNCONFIRMED : 0u;
    }
}

// One lane per proof of the single-output class (launch position i = gathered position i: the class comes first):
// conf[i] = 0 when V_0 of its decoded record is amounts[caller] g + masks[i] h, else 1.  A lane whose container the decoder
// rejected (status[i]: its record may never have been written) or whose Gamma is undefined (conf[i] already
// BPP_SCAN_UNCONFIRMED, from k_recover_masks) returns before its first load.  records: the class region, nv wire points per
// record, V_0 the v0-th.  The Edwards instantiation compares ristretto255 ELEMENTS (a decoded point is any
// representative of its coset, ristretto.hpp), the other curves the wire images.
template <class C>
__global__ void __launch_bounds__(COMMIT_BLOCK) k_recover_confirm(VerifyShape s, const uint32_t* __restrict__ table,
                                                                  const uint32_t* __restrict__ rx,
                                                                  const uint64_t* __restrict__ amounts,
                                                                  const uint32_t* __restrict__ masks, uint32_t amount64,
                                                                  const uint32_t* __restrict__ records, uint32_t nv, uint32_t v0,
                                                                  const uint32_t* __restrict__ status, uint32_t* __restrict__ conf,
                                                                  size_t count) {
    constexpr int N = C::Fp::N;
    constexpr int WW = 2 * N + 2;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count || status[i] || conf[i] == BPP_SCAN_UNCONFIRMED) return;
    // the lane of k_commit_batch (commit.hpp), statement for statement: the scalars, the walk, the wire image
    using P = typename C::Fr;
    uint32_t kv[8], kg[8];
    commit_amount_scalar<C>(amounts[rx[i * RX_WORDS + RX_CALLER]], amount64 != 0, kv);
    ld_words<8>(masks + i * 8, kg);
    fe_to_canonical(fe_from_canonical<P>(kg), kg);
    const Xyzz<C> acc = commit_walk<C>(
        s, kv, kg, [&](size_t e) { return aff_ldg<C>(table + e * (size_t)(2 * N)); },
        [](Xyzz<C>& a, const Aff<C>& q, bool neg) { xyzz_madd_lazy(a, q, neg); });
    uint32_t w[WW];
    aff_to_wire(jac_to_aff(xyzz_to_jac(acc)), w);
    const uint32_t* V = records + ((size_t)i * nv + v0) * WW;
    const bool inf_w = (w[2 * N] | w[2 * N + 1]) != 0, inf_V = (V[2 * N] | V[2 * N + 1]) != 0;
    bool same;
    if constexpr (C::ID == 2) {
        using Fp = typename C::Fp;
        Aff<C> a = aff_inf<C>(), b = aff_inf<C>();
        if (!inf_w) {
            a.x = fe_from_canonical<Fp>(w);
            a.y = fe_from_canonical<Fp>(w + N);
        }
        if (!inf_V) {
            b.x = fe_from_canonical<Fp>(V);
            b.y = fe_from_canonical<Fp>(V + N);
        }
        same = rist_equal(a, b);
    } else {
        same = inf_w == inf_V;
        if (!inf_w)
            for (int t = 0; t < 2 * N; t++) same = same && w[t] == V[t];
    }
    conf[i] = same ? 0u : 1u;
}

// From gathered position back to caller position, one lane per proof: the status word -- 2 where the decoder rejected the
// container, for the first n_conf positions the confirmation's 0 / 1 or BPP_SCAN_UNCONFIRMED after a zero challenge, else
// BPP_SCAN_UNCONFIRMED -- and Gamma, zero under status 1 and 2.
template <class C>
__global__ void __launch_bounds__(256) k_recover_scatter(const uint32_t* __restrict__ rx, const uint32_t* __restrict__ status,
                                                         const uint32_t* __restrict__ conf, size_t n_conf,
                                                         const uint32_t* __restrict__ masks, uint32_t* __restrict__ out_masks,
                                                         uint32_t* __restrict__ out_status, size_t count) {
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= count) return;
    const size_t caller = rx[pos * RX_WORDS + RX_CALLER];
    const uint32_t st = status[pos] ? (uint32_t)BPP_FORMAT_ERROR : pos < n_conf ? conf[pos] : (uint32_t)BPP_SCAN_UNCONFIRMED;
    uint32_t o[8];
    ld_words<8>(masks + pos * 8, o);
    if (st == BPP_VERIFICATION_ERROR || st == BPP_FORMAT_ERROR)
        for (int t = 0; t < 8; t++) o[t] = 0;
    st_words<8>(out_masks + caller * 8, o);
    out_status[caller] = st;
}

template <class C>
struct RecoverImpl {
    using V = VerifyImpl<C>;
    static constexpr int WW = 2 * C::Fp::N + 2;

    // the wire call's per-proof entries by gathered position, for a plan of mixed_plan
    static void build_rx(const VerifyShape& cap, const MixedPlan& p, const uint32_t* m_of, size_t count, std::vector<uint32_t>& rx);
    // the call's part of a job: the blinding source of the record (a.index, a.blinding: the device's)
    static RecoverJob call_job(const ScanArgs& a);
    // one class: count proofs of class c from gathered position first.  j: the call's part, the per-proof entries from
    // gathered position 0 and the launch's buffers (triples, ch, out, conf and how they are addressed)
    static int launch_recover(const bpp_verifier* v, uint32_t c, size_t first, size_t count, RecoverJob j, hipStream_t st);
    // a class of the plan whose term count does not fit a lane group: BPP_E_ARG (none with today's make_shape)
    static int check_classes(const bpp_verifier* v, const MixedPlan& p) {
        for (uint32_t c = 0; c < MIXED_CLASSES; c++)
            if (p.count[c] && V::class_shape(v, c).s.k + 2 > RECOVER_GROUP)
                return fail(BPP_E_ARG, "mask recovery takes shapes with log2(n m) <= 14");
        return BPP_OK;
    }

    // ---- recovery from wire data: triples and challenge blocks in caller order, no points --------------------------------
    // workspace = the per-proof entries.  0 for an m_of the verifier does not take.
    static size_t recover_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count);
    // a.scalars: count x 3 ; a.challenges: the packed 3 + k_i blocks, or null: the literals of each proof's own shape;
    // a.out_masks: count x 4 words of Gamma_i, caller order.  Uploads the per-proof entries (blocking the host until the copy
    // has read them); per class present one launch of k_recover_masks that reads and writes the caller's buffers through
    // the entries -- nothing is gathered and nothing scattered.
    static int recover_masks_mixed(bpp_verifier* v, const ScanArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);
    // host buffers in, host buffers out (blinding, index: host, may be null): the record with the device's pointers swapped in
    static int recover_masks_mixed_host(bpp_verifier* v, const ScanArgs& a);

    // ---- scanning from bytes: run_serialized_mixed's front (decoder, membership test, challenges), then recovery and the
    // confirmation instead of the verifier's pass ----------------------------------------------------------------------
    // workspace = front (MixedFront, serialized form; its index is the one per-proof table) | Gamma and confirmation by
    // gathered position
    struct ScanLayout {
        typename V::MixedFront f;
        size_t masks, conf, total;
    };
    static ScanLayout scan_layout(const MixedPlan& p, size_t count) {
        ScanLayout w;
        WsCarver o;
        w.f = V::carve_front(o, p, count, true);
        w.masks = o.take(count * 32);
        w.conf = o.take(count * 4);
        w.total = o.total;
        return w;
    }
    static size_t scan_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count);
    // a.proofs, a.commitments, a.m_of, a.version: run_serialized_mixed's; a.amounts: count x u64 by caller position, or null;
    // a.out_masks: count x 4 words, a.out_status: count words, caller order
    static int scan_serialized_mixed(bpp_verifier* v, const ScanArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);
    static int scan_serialized_mixed_host(bpp_verifier* v, const ScanArgs& a);
};

// Where proof i's blinding scalars sit in a call's packed buffer (in scalars: 5 + 2 k_i of them, k_i = log2(n m_i)): into
// at[i] when at is given; returns their total.
inline size_t blind_offsets(const VerifyShape& cap, const uint32_t* m_of, size_t count, uint32_t* at = nullptr) {
    const uint32_t logn = cap.k - (uint32_t)__builtin_ctz(cap.m);
    size_t total = 0;
    for (size_t i = 0; i < count; i++) {
        if (at) at[i] = (uint32_t)total;
        total += pb_blind_elems(logn + (uint32_t)__builtin_ctz(m_of[i]));
    }
    return total;
}

#ifdef BPP_IMPL_DEFINITIONS
template <class C>
void RecoverImpl<C>::build_rx(const VerifyShape& cap, const MixedPlan& p, const uint32_t* m_of, size_t count,
                              std::vector<uint32_t>& rx) {
    const uint32_t logn = cap.k - (uint32_t)__builtin_ctz(cap.m);
    rx.assign(count * RX_WORDS, 0u);
    std::vector<uint32_t> at(count);
    blind_offsets(cap, m_of, count, at.data());
    size_t next[MIXED_CLASSES];
    for (uint32_t c = 0; c < MIXED_CLASSES; c++) next[c] = p.first[c];
    size_t src_ch = 0;
    for (size_t i = 0; i < count; i++) {
        const uint32_t c = (uint32_t)__builtin_ctz(m_of[i]);
        uint32_t* e = rx.data() + next[c]++ * RX_WORDS;
        e[RX_CALLER] = (uint32_t)i;
        e[RX_BLIND] = at[i];
        e[RX_CH] = (uint32_t)src_ch;
        src_ch += 3 + logn + c;
    }
}

template <class C>
RecoverJob RecoverImpl<C>::call_job(const ScanArgs& a) {
    RecoverJob j = {};
    load_key_words(a.blind_key, j.key.w);
    j.have_key = a.blind_key ? 1u : 0u;
    j.index_base = a.index_base;
    j.index = a.index;
    j.blinding = reinterpret_cast<const uint32_t*>(a.blinding);
    return j;
}

template <class C>
int RecoverImpl<C>::launch_recover(const bpp_verifier* v, uint32_t c, size_t first, size_t count, RecoverJob j, hipStream_t st) {
    const VerifyShape& s = V::class_shape(v, c).s;
    j.k = s.k;
    j.m = s.m;
    // alpha: range/mod.rs:94 / :256 ; d_L, d_R: wip.rs:94-95 ; delta, eta: wip.rs:177-178
    j.lit = recover_literals(s.m == 1 ? 7 : 33, 4, 5, 88, 123);
    j.rx += first * RX_WORDS;
    j.count = count;
    hipLaunchKernelGGL(k_recover_masks<C>, dim3(cdiv(count * RECOVER_GROUP, RECOVER_BLOCK)), dim3(RECOVER_BLOCK), 0, st, j);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
size_t RecoverImpl<C>::recover_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count) {
    MixedPlan p;
    if (mixed_plan(v->s, m_of, count, false, p)) return 0;
    WsCarver o;
    o.take(count * (size_t)RX_WORDS * 4);
    return o.total;
}

template <class C>
int RecoverImpl<C>::recover_masks_mixed(bpp_verifier* v, const ScanArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
    MixedPlan p;
    int rc = mixed_plan(v->s, a.m_of, a.count, false, p);
    if (rc) return rc;
    if (workspace_bytes < recover_workspace_bytes(v, a.m_of, a.count)) return fail(BPP_E_ARG, "workspace too small");
    if ((rc = check_classes(v, p))) return rc;
    std::vector<uint32_t> rx;
    build_rx(v->s, p, a.m_of, a.count, rx);
    uint32_t* d_rx = static_cast<uint32_t*>(d_workspace);
    // pageable source: the copy has read it when the call returns
    HIPCHK(hipMemcpyAsync(d_rx, rx.data(), rx.size() * 4, hipMemcpyHostToDevice, st));
    // the launches read and write the caller's buffers, by caller position
    RecoverJob j = call_job(a);
    j.rx = d_rx;
    j.triples = reinterpret_cast<const uint32_t*>(a.scalars);
    j.triples_by_caller = 1u;
    j.out = reinterpret_cast<uint32_t*>(a.out_masks);
    j.out_by_caller = 1u;
    j.ch_mode = a.challenges ? RCH_INDEXED : RCH_SHARED;
    for (uint32_t c = 0; c < MIXED_CLASSES; c++) {
        if (!p.count[c]) continue;
        j.ch = a.challenges ? reinterpret_cast<const uint32_t*>(a.challenges) : V::class_shape(v, c).challenges;
        if ((rc = launch_recover(v, c, p.first[c], p.count[c], j, st))) return rc;
    }
    return BPP_OK;
}

// what every host twin of a scan uploads of its block: proofs, commitments, index and amounts (n_amounts of them)
struct BlockUpload {
    DevBuf proofs, commitments, index, amounts;
    int upload(const MixedPlan& p, const uint8_t* h_proofs, const uint8_t* h_commitments, const uint64_t* h_index, size_t count,
               const uint64_t* h_amounts, size_t n_amounts) {
        HIPCHK(proofs.upload(h_proofs, p.proof_bytes));
        HIPCHK(commitments.upload(h_commitments, p.comm_bytes));
        HIPCHK(index.upload(h_index, count * 8));
        HIPCHK(amounts.upload(h_amounts, n_amounts * 8));
        return BPP_OK;
    }
    // a scan's record with what was uploaded in the host pointers' place
    ScanArgs device_args(const ScanArgs& a) const {
        ScanArgs d = a;
        d.proofs = proofs.u8();
        d.commitments = commitments.u8();
        d.index = index.u64();
        d.amounts = amounts.u64();
        return d;
    }
};

template <class C>
int RecoverImpl<C>::recover_masks_mixed_host(bpp_verifier* v, const ScanArgs& a) {
    const size_t count = a.count;
    MixedPlan p;
    int rc = mixed_plan(v->s, a.m_of, count, false, p);
    if (rc) return rc;
    DevBuf dsc, dch, dix, dbl, dout, dws;
    HIPCHK(dsc.upload(a.scalars, count * 96));
    HIPCHK(dch.upload(a.challenges, p.chals * 32));
    HIPCHK(dix.upload(a.index, count * 8));
    HIPCHK(dbl.upload(a.blinding, blind_offsets(v->s, a.m_of, count) * 32));
    const size_t wsb = recover_workspace_bytes(v, a.m_of, count);
    HIPCHK(dout.alloc(count * 32));
    HIPCHK(dws.alloc(wsb));
    ScanArgs d = a;
    d.scalars = dsc.u64();
    d.challenges = dch.u64();
    d.index = dix.u64();
    d.blinding = dbl.u64();
    d.out_masks = dout.u64();
    BPP_TRY(recover_masks_mixed(v, d, dws.p, wsb, nullptr));
    HIPCHK(dout.download(a.out_masks, count * 32));
    return BPP_OK;
}

template <class C>
size_t RecoverImpl<C>::scan_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count) {
    MixedPlan p;
    if (!V::container_shape_ok(v) || mixed_plan_serialized(v->s, m_of, count, max_point_bytes<C>(), false, p)) return 0;
    return scan_layout(p, count).total;
}

template <class C>
int RecoverImpl<C>::scan_serialized_mixed(bpp_verifier* v, const ScanArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
    if (int rc = V::container_args_ok(v, a.version)) return rc;
    const size_t count = a.count;
    MixedPlan p;
    int rc = mixed_plan_serialized(v->s, a.m_of, count, (size_t)container_point_bytes<C>(a.version), true, p);
    if (rc) return rc;
    const ScanLayout L = scan_layout(p, count);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    if ((rc = check_classes(v, p))) return rc;
    if (a.blinding) {   // where each proof's blinding scalars sit, into the free word of the decoder's index
        std::vector<uint32_t> at(count);
        blind_offsets(v->s, a.m_of, count, at.data());
        for (size_t pos = 0; pos < count; pos++) p.sidx[pos * SX_WORDS + RX_BLIND] = at[p.sidx[pos * SX_WORDS + SX_CALLER]];
    }
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    const uint32_t* w_idx = W(L.f.idx);
    rc = V::decode_front(p, L.f, count, a.proofs, a.commitments, a.version, ws, st);
    if (rc) return rc;
    // the launches read the decoded class regions and write Gamma and the confirmation word, by launch position
    RecoverJob j = call_job(a);
    j.rx = w_idx;
    j.ch_mode = a.fs ? RCH_STRIDED : RCH_SHARED;
    size_t n_conf = 0;
    rc = V::for_each_class(v, p, L.f, ws, [&](const typename V::ClassView& cv) {
        if (a.fs) {
            const int rc1 = V::derive_challenges(v, cv.ps, cv.pts, cv.count, cv.challenges, st);
            if (rc1) return rc1;
        }
        j.triples = reinterpret_cast<const uint32_t*>(cv.sc3);
        j.ch = a.fs ? reinterpret_cast<const uint32_t*>(cv.challenges) : cv.ps.challenges;
        j.out = W(L.masks) + cv.first * 8;
        j.conf = W(L.conf) + cv.first;
        const int rc2 = launch_recover(v, cv.c, cv.first, cv.count, j, st);
        if (rc2 || cv.c != 0 || !a.amounts) return rc2;
        // the single-output class comes first in gathered order: launch position = gathered position
        n_conf = cv.count;
        hipLaunchKernelGGL(k_recover_confirm<C>, dim3(cdiv(cv.count, COMMIT_BLOCK)), dim3(COMMIT_BLOCK), 0, st, v->s,
                           v->table.u32(), w_idx, a.amounts, W(L.masks), a.amount64 ? 1u : 0u,
                           reinterpret_cast<const uint32_t*>(cv.pts), cv.ps.s.NV, 3 + 2 * cv.ps.s.k, W(L.f.status), W(L.conf),
                           cv.count);
        HIPCHK(hipGetLastError());
        return BPP_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_recover_scatter<C>, dim3(cdiv(count, 256)), dim3(256), 0, st, w_idx, W(L.f.status), W(L.conf), n_conf,
                       W(L.masks), reinterpret_cast<uint32_t*>(a.out_masks), a.out_status, count);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int RecoverImpl<C>::scan_serialized_mixed_host(bpp_verifier* v, const ScanArgs& a) {
    if (int rc = V::container_args_ok(v, a.version)) return rc;
    const size_t count = a.count;
    MixedPlan p;
    int rc = mixed_plan_serialized(v->s, a.m_of, count, (size_t)container_point_bytes<C>(a.version), false, p);
    if (rc) return rc;
    BlockUpload up;
    DevBuf dbl, dout, dst, dws;
    BPP_TRY(up.upload(p, a.proofs, a.commitments, a.index, count, a.amounts, count));
    HIPCHK(dbl.upload(a.blinding, blind_offsets(v->s, a.m_of, count) * 32));
    const size_t wsb = scan_layout(p, count).total;
    HIPCHK(dout.alloc(count * 32));
    HIPCHK(dst.alloc(count * 4));
    HIPCHK(dws.alloc(wsb));
    ScanArgs d = up.device_args(a);
    d.blinding = dbl.u64();
    d.out_masks = dout.u64();
    d.out_status = dst.u32();
    BPP_TRY(scan_serialized_mixed(v, d, dws.p, wsb, nullptr));
    HIPCHK(dout.download(a.out_masks, count * 32));
    HIPCHK(dst.download(a.out_status, count * 4));
    return BPP_OK;
}
#endif  // BPP_IMPL_DEFINITIONS

extern template struct RecoverImpl<Bls12381>;
extern template struct RecoverImpl<Secp256k1>;
extern template struct RecoverImpl<Ed25519>;

}  // namespace bpp
