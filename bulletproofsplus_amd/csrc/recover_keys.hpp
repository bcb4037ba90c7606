// recover_keys.hpp -- scanning a block of containers under MANY blinding keys in one call
// (bpp_range_scan_serialized_mixed_keys*): the front of the single-key scan (recover.hpp) once, the inversions once per
// proof, and per (key, proof) pair only what depends on the key.  recover_coeffs.hpp has the arithmetic.  One
// instantiation per curve (tu_recover_keys_*.hip).
//
// k_recover_coeffs: k_recover_masks's mapping -- a proof is RECOVER_GROUP = 16 lanes, lane t inverts for term t (t < k:
// e_t^2; t = k: e^2 y^(nm+1) [z^2]) -- but what is written is the proof's 2k + 4 coefficients, by gathered position, and
// a flag for a zero challenge.  Nothing of a key is involved: the coefficients are public and live in the workspace, as
// the field's own limbs (Montgomery form, COEFF_WORDS words each) so that a pair lane multiplies what it loads.
// k_scan_keys: a pair is SCAN_GROUP = 8 lanes, eight pairs per wave; lane s expands live slots s, s + 8, s + 16 and, for
// k >= 11 (25 live slots at k = 11, 27 at k = 12), s + 24 in a fourth stride (alpha, delta, eta, d_L, d_R: 2k + 3 of
// them; r and s have coefficient zero and are never hashed), multiplies each by its coefficient, the group sums by a
// 3-step butterfly of wave_shfl and lane 0 adds A0 and stores Gamma and the status at [key][caller position].
// The key's words come from the caller's buffer into registers; no LDS, no scratch, no atomics:
// nothing derived from a key but Gamma reaches memory.  Pairs are numbered proof-major (pair = position * n_keys + key),
// so the groups of a wave read one proof's coefficients.
// k_scan_keys_confirm: one lane per (key, single-output proof) pair with a candidate amount: k_recover_confirm's walk,
// compared with the decoded V_0 projectively (walk_equals_wire): no inversion in Fp.
// What a pair's lanes compute is written once, as force-inlined device functions -- pair_key_index, pair_gamma,
// pair_confirms -- which the find kernels (find.hpp) call too; a kernel keeps its numbering, its early exits and its stores.
// Force-inlined because the key is a local array: handed to a function that is not inlined it would go through memory.
#pragma once
#include "recover.hpp"
#include "recover_coeffs.hpp"

namespace bpp {

constexpr unsigned SCAN_GROUP = 8;   // lanes per (key, proof) pair
constexpr unsigned SCAN_BLOCK = 64;
// a coefficient in memory: the NL limbs of the scalar field, padded to whole 16-byte granules
template <class P>
constexpr int coeff_words() {
    return (P::NL + 3) & ~3;
}

template <class P>
__device__ __forceinline__ Fe<P> coeff_ldg(const uint32_t* __restrict__ p) {
    uint32_t w[coeff_words<P>()];
    ld_words<coeff_words<P>()>(p, w);
    Fe<P> r;
#pragma unroll
    for (int i = 0; i < P::NL; i++) r.l[i] = w[i];
    return r;
}
template <class P>
__device__ __forceinline__ void coeff_stg(uint32_t* __restrict__ p, const Fe<P>& a) {
    uint32_t w[coeff_words<P>()];
#pragma unroll
    for (int i = 0; i < coeff_words<P>(); i++) w[i] = i < P::NL ? a.l[i] : 0u;
    st_words<coeff_words<P>()>(p, w);
}

// One class: `count` proofs of shape (n, m), k = log2(n m); triples and challenge blocks (3 + k scalars per proof) by
// launch position.  coeffs: count x coeff_elems(k) x COEFF_WORDS; bad[i] = 1 after a zero challenge, else 0.
template <class C>
__global__ void __launch_bounds__(RECOVER_BLOCK) k_recover_coeffs(uint32_t k, uint32_t m, const uint32_t* __restrict__ triples,
                                                                  const uint32_t* __restrict__ ch, uint32_t* __restrict__ coeffs,
                                                                  uint32_t* __restrict__ bad_out, size_t count) {
    using P = typename C::Fr;
    using F = Fe<P>;
    constexpr int CW = coeff_words<P>();
    const uint32_t lane = threadIdx.x & 63u, t = lane & (RECOVER_GROUP - 1);
    const size_t g = ((size_t)blockIdx.x * RECOVER_BLOCK + threadIdx.x) / RECOVER_GROUP;
    const bool live = g < count;
    const size_t p = live ? g : count - 1;   // an idle group of the last wave repeats the last proof and stores nothing
    const uint32_t* pch = ch + p * (size_t)(3 + k) * 8;
    F e = F::zero(), e2 = F::zero(), den = F::zero();
    bool ok;
    const F x = coeff_term_x<P>(k, m, t, pch, e, e2, den, ok);
    const F xinv = fe_inv(x);
    F D = F::one(), head[4];
    if (t == k) {
        uint32_t w[8];
        ld_words<8>(triples + p * 24 + 16, w);
        coeff_head(fe_from_canonical<P>(w), e, e2, den, xinv, D, head);
    }
    D = wave_shfl(D, (int)((lane & ~(RECOVER_GROUP - 1)) + k));
    uint32_t bad = ok ? 0u : 1u;
#pragma unroll 1
    for (int d = RECOVER_GROUP >> 1; d >= 1; d >>= 1) bad |= (uint32_t)__shfl((int)bad, (int)(lane ^ d), 64);
    if (!live) return;
    uint32_t* o = coeffs + p * (size_t)coeff_elems(k) * CW;
    if (t < k) {
        F cL, cR;
        coeff_round(D, x, xinv, cL, cR);
        coeff_stg<P>(o + (size_t)(4 + t) * CW, cL);
        coeff_stg<P>(o + (size_t)(4 + k + t) * CW, cR);
    } else if (t == k) {
#pragma unroll
        for (int h = 0; h < 4; h++) coeff_stg<P>(o + (size_t)h * CW, head[h]);
        bad_out[p] = bad;
    }
}

// one launch of the pair kernels: `count` proofs of one class (rx: their entries, by launch position) under n_keys keys
struct ScanKeysJob {
    uint32_t k;
    uint32_t n_keys;
    const uint32_t* keys;        // the CALLER's buffer: n_keys x 8 little-endian words
    uint64_t index_base;
    const uint64_t* index;       // by caller position, or null: index_base + caller position
    const uint32_t* rx;
    const uint32_t* coeffs;
    const uint32_t* bad;
    const uint32_t* status;      // the decoder's, by launch position
    uint32_t* out_masks;         // n_keys x total x 8 words, [key][caller position]
    uint32_t* out_status;        // n_keys x total
    size_t count, total;         // proofs of this class, proofs of the call
};

// key number key_no's eight words from a buffer of keys into registers: the one place a kernel reads a key
__device__ __forceinline__ void load_key(const uint32_t* keys, size_t key_no, uint32_t key[8]) {
#pragma unroll
    for (int w = 0; w < 8; w++) key[w] = keys[key_no * 8 + w];
}

// key number key_no's words from the caller's buffer into registers; returns the blinding index of caller position `caller`
__device__ __forceinline__ uint64_t pair_key_index(const ScanKeysJob& j, size_t key_no, size_t caller, uint32_t key[8]) {
    load_key(j.keys, key_no, key);
    return j.index ? j.index[caller] : j.index_base + caller;
}

// Gamma = A0 + sum c_s slot_s of the pair (key key_no, launch position p, caller position `caller`), by the pair's whole
// group of SCAN_GROUP lanes: a strided sum over the live slots, the butterfly, and from lane s == 0 the canonical words to
// the pair's place `at` of j.out_masks
template <class C>
__device__ __forceinline__ void pair_gamma(const ScanKeysJob& j, size_t key_no, size_t p, size_t caller, size_t at) {
    using P = typename C::Fr;
    using F = Fe<P>;
    constexpr int CW = coeff_words<P>();
    const uint32_t lane = threadIdx.x & 63u, s = lane & (SCAN_GROUP - 1);
    uint32_t key[8];
    const uint64_t idx = pair_key_index(j, key_no, caller, key);
    const uint32_t nl = coeff_live_slots(j.k);
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
        st_words<8>(j.out_masks + at * 8, o);
    }
}

// whether V_0 of the record of launch position p is amount g + Gamma h, with the canonical Gamma a scan kernel left at
// pair place `at`: k_recover_confirm's walk, compared projectively
template <class C>
__device__ __forceinline__ bool pair_confirms(const VerifyShape& s, const uint32_t* __restrict__ table, const ScanKeysJob& j,
                                              uint64_t amount, uint32_t amount64, size_t at, size_t p,
                                              const uint32_t* __restrict__ records, uint32_t nv, uint32_t v0) {
    constexpr int N = C::Fp::N;
    constexpr int WW = 2 * N + 2;
    uint32_t kv[8], kg[8];
    commit_amount_scalar<C>(amount, amount64 != 0, kv);
    ld_words<8>(j.out_masks + at * 8, kg);
    const Xyzz<C> acc = commit_walk<C>(
        s, kv, kg, [&](size_t e) { return aff_ldg<C>(table + e * (size_t)(2 * N)); },
        [](Xyzz<C>& a, const Aff<C>& pt, bool neg) { xyzz_madd_lazy(a, pt, neg); });
    return walk_equals_wire<C>(acc, records + ((size_t)p * nv + v0) * WW);
}

template <class C>
__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_keys(ScanKeysJob j) {
    const uint32_t s = threadIdx.x & (SCAN_GROUP - 1);
    const size_t q = ((size_t)blockIdx.x * SCAN_BLOCK + threadIdx.x) / SCAN_GROUP;
    if (q >= j.count * j.n_keys) return;   // a whole group: the exchanges of pair_gamma stay inside a group
    const size_t p = q / j.n_keys;
    const uint32_t key_no = (uint32_t)(q - p * j.n_keys);
    const size_t caller = j.rx[p * RX_WORDS + RX_CALLER];
    const size_t at = (size_t)key_no * j.total + caller;
    const bool rejected = j.status[p] != 0;
    if (rejected || j.bad[p]) {   // before the key is read: the decoder's FormatError for every key; Gamma undefined
        if (s == 0) {
            const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            st_words<8>(j.out_masks + at * 8, z);
            j.out_status[at] = rejected ? (uint32_t)BPP_FORMAT_ERROR : (uint32_t)BPP_SCAN_UNCONFIRMED;
        }
        return;
    }
    pair_gamma<C>(j, key_no, p, caller, at);
    if (s == 0) j.out_status[at] = (uint32_t)BPP_SCAN_UNCONFIRMED;
}

// One lane per (key, proof) pair of the single-output class (launch position = gathered position: the class comes
// first), numbered as k_scan_keys numbers them: status 0 when V_0 of the proof's decoded record is
// amounts[key][caller] g + Gamma h with the Gamma k_scan_keys left at [key][caller], else status 1 and Gamma zeroed.  A
// lane whose container the decoder rejected or whose coefficients are undefined returns before its first load of either.
template <class C>
__global__ void __launch_bounds__(COMMIT_BLOCK) k_scan_keys_confirm(VerifyShape s, const uint32_t* __restrict__ table,
                                                                    ScanKeysJob j, const uint64_t* __restrict__ amounts,
                                                                    uint32_t amount64, const uint32_t* __restrict__ records,
                                                                    uint32_t nv, uint32_t v0) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= j.count * j.n_keys) return;
    const size_t p = q / j.n_keys;
    if (j.status[p] || j.bad[p]) return;
    const size_t at = (q - p * j.n_keys) * j.total + j.rx[p * RX_WORDS + RX_CALLER];
    const bool same = pair_confirms<C>(s, table, j, amounts[at], amount64, at, p, records, nv, v0);
    j.out_status[at] = same ? 0u : 1u;
    if (!same) {
        const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        st_words<8>(j.out_masks + at * 8, z);
    }
}

template <class C>
struct RecoverKeysImpl {
    using V = VerifyImpl<C>;
    using R = RecoverImpl<C>;
    static constexpr int CW = coeff_words<typename C::Fr>();

    // workspace = front (MixedFront, serialized form) | coefficients, class after class by gathered position | the
    // zero-challenge flags by gathered position.  Its size does not depend on the number of keys.
    struct Layout {
        typename V::MixedFront f;
        size_t coeffs, coeff_of[MIXED_CLASSES], bad, total;
    };
    static Layout layout(const bpp_verifier* v, const MixedPlan& p, size_t count) {
        Layout w;
        WsCarver o;
        w.f = V::carve_front(o, p, count, true);
        size_t elems = 0;
        for (uint32_t c = 0; c < MIXED_CLASSES; c++) {
            w.coeff_of[c] = elems;
            if (p.count[c]) elems += p.count[c] * coeff_elems(V::class_shape(v, c).s.k);
        }
        w.coeffs = o.take(elems * CW * 4);
        w.bad = o.take(count * 4);
        w.total = o.total;
        return w;
    }
    static size_t workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count);
    // the call's part of the pair job: the keys, the index and total; where Gamma and the pair word go ([key][caller
    // position]: out_masks, out_status) is the caller's to add
    static ScanKeysJob call_job(const uint8_t* d_keys, size_t n_keys, uint64_t index_base, const uint64_t* d_index, size_t total);
    // One class of a call, in three steps (the find call, find.hpp, takes them apart).  bind_class: the class's part of j
    // (k, rx, coeffs, bad, status, count), which the confirmation that follows reads too; w_idx, w_status, w_bad: the call's,
    // from gathered position 0; coeffs: the class's.  launch_coeffs: k_recover_coeffs over its proofs, into the coeffs and
    // bad that j was bound to.  launch_scan_keys: k_scan_keys over its (key, proof) pairs.
    static void bind_class(const typename V::ClassView& cv, const uint32_t* w_idx, const uint32_t* w_status, const uint32_t* w_bad,
                           const uint32_t* coeffs, ScanKeysJob& j);
    static int launch_coeffs(const typename V::ClassView& cv, uint32_t* coeffs, uint32_t* w_bad, hipStream_t st);
    static int launch_scan_keys(const ScanKeysJob& j, hipStream_t st);
    // a.keys: n_keys x 32 bytes (device, 4-byte aligned); a.index: count x u64 or null; a.amounts: n_keys x count or null;
    // a.out_masks: n_keys x count x 4 words; a.out_status: n_keys x count words
    static int scan(bpp_verifier* v, const ScanArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);
    static int scan_host(bpp_verifier* v, const ScanArgs& a);
};

#ifdef BPP_IMPL_DEFINITIONS
template <class C>
size_t RecoverKeysImpl<C>::workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count) {
    MixedPlan p;
    if (!V::container_shape_ok(v) || mixed_plan_serialized(v->s, m_of, count, max_point_bytes<C>(), false, p)) return 0;
    return layout(v, p, count).total;
}

template <class C>
int RecoverKeysImpl<C>::scan(bpp_verifier* v, const ScanArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
    if (int rc = V::container_args_ok(v, a.version)) return rc;
    const size_t count = a.count, n_keys = a.n_keys;
    MixedPlan p;
    int rc = mixed_plan_serialized(v->s, a.m_of, count, (size_t)container_point_bytes<C>(a.version), true, p);
    if (rc) return rc;
    const Layout L = layout(v, p, count);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    if ((rc = R::check_classes(v, p))) return rc;
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    rc = V::decode_front(p, L.f, count, a.proofs, a.commitments, a.version, ws, st);
    if (rc) return rc;
    ScanKeysJob j = call_job(a.keys, n_keys, a.index_base, a.index, count);
    j.out_masks = reinterpret_cast<uint32_t*>(a.out_masks);
    j.out_status = a.out_status;
    return V::for_each_class(v, p, L.f, ws, [&](const typename V::ClassView& cv) {
        int rc1 = V::derive_challenges(v, cv.ps, cv.pts, cv.count, cv.challenges, st);
        if (rc1) return rc1;
        uint32_t* coeffs = W(L.coeffs) + L.coeff_of[cv.c] * CW;
        bind_class(cv, W(L.f.idx), W(L.f.status), W(L.bad), coeffs, j);
        if ((rc1 = launch_coeffs(cv, coeffs, W(L.bad), st))) return rc1;
        if ((rc1 = launch_scan_keys(j, st))) return rc1;
        if (cv.c != 0 || !a.amounts) return BPP_OK;
        // the single-output class comes first in gathered order: launch position = gathered position
        hipLaunchKernelGGL(k_scan_keys_confirm<C>, dim3(cdiv(cv.count * n_keys, COMMIT_BLOCK)), dim3(COMMIT_BLOCK), 0, st, v->s,
                           v->table.u32(), j, a.amounts, a.amount64 ? 1u : 0u, reinterpret_cast<const uint32_t*>(cv.pts),
                           cv.ps.s.NV, 3 + 2 * cv.ps.s.k);
        HIPCHK(hipGetLastError());
        return BPP_OK;
    });
}

template <class C>
ScanKeysJob RecoverKeysImpl<C>::call_job(const uint8_t* d_keys, size_t n_keys, uint64_t index_base, const uint64_t* d_index,
                                         size_t total) {
    ScanKeysJob j = {};
    j.n_keys = (uint32_t)n_keys;
    j.keys = reinterpret_cast<const uint32_t*>(d_keys);
    j.index_base = index_base;
    j.index = d_index;
    j.total = total;
    return j;
}

template <class C>
void RecoverKeysImpl<C>::bind_class(const typename V::ClassView& cv, const uint32_t* w_idx, const uint32_t* w_status,
                                    const uint32_t* w_bad, const uint32_t* coeffs, ScanKeysJob& j) {
    j.k = cv.ps.s.k;
    j.rx = w_idx + cv.first * RX_WORDS;
    j.coeffs = coeffs;
    j.bad = w_bad + cv.first;
    j.status = w_status + cv.first;
    j.count = cv.count;
}

template <class C>
int RecoverKeysImpl<C>::launch_coeffs(const typename V::ClassView& cv, uint32_t* coeffs, uint32_t* w_bad, hipStream_t st) {
    hipLaunchKernelGGL(k_recover_coeffs<C>, dim3(cdiv(cv.count * RECOVER_GROUP, RECOVER_BLOCK)), dim3(RECOVER_BLOCK), 0, st,
                       cv.ps.s.k, cv.ps.s.m, reinterpret_cast<const uint32_t*>(cv.sc3),
                       reinterpret_cast<const uint32_t*>(cv.challenges), coeffs, w_bad + cv.first, cv.count);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int RecoverKeysImpl<C>::launch_scan_keys(const ScanKeysJob& j, hipStream_t st) {
    hipLaunchKernelGGL(k_scan_keys<C>, dim3(cdiv(j.count * j.n_keys * SCAN_GROUP, SCAN_BLOCK)), dim3(SCAN_BLOCK), 0, st, j);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int RecoverKeysImpl<C>::scan_host(bpp_verifier* v, const ScanArgs& a) {
    if (int rc = V::container_args_ok(v, a.version)) return rc;
    const size_t count = a.count;
    MixedPlan p;
    int rc = mixed_plan_serialized(v->s, a.m_of, count, (size_t)container_point_bytes<C>(a.version), false, p);
    if (rc) return rc;
    const size_t pairs = a.n_keys * count;
    DevBuf dk(true);   // the keys: wiped before they are freed, on every way out
    BlockUpload up;
    DevBuf dout, dst, dws;
    BPP_TRY(up.upload(p, a.proofs, a.commitments, a.index, count, a.amounts, pairs));
    HIPCHK(dk.upload(a.keys, a.n_keys * 32));
    const size_t wsb = layout(v, p, count).total;
    HIPCHK(dout.alloc(pairs * 32));
    HIPCHK(dst.alloc(pairs * 4));
    HIPCHK(dws.alloc(wsb));
    ScanArgs d = up.device_args(a);
    d.keys = dk.u8();
    d.out_masks = dout.u64();
    d.out_status = dst.u32();
    BPP_TRY(scan(v, d, dws.p, wsb, nullptr));
    HIPCHK(dout.download(a.out_masks, pairs * 32));
    HIPCHK(dst.download(a.out_status, pairs * 4));
    return BPP_OK;
}
#endif  // BPP_IMPL_DEFINITIONS

extern template struct RecoverKeysImpl<Bls12381>;
extern template struct RecoverKeysImpl<Secp256k1>;
extern template struct RecoverKeysImpl<Ed25519>;

}  // namespace bpp
