// recover_terms.hpp -- the arithmetic of mask recovery ("rewind"): what the holder of a proof's blinding scalars gets back
// out of its last scalar delta'.  Plain C++ on field.hpp and sha256.hpp, so the host test
// (tests/host/recover_host_test.cpp) compiles the very code k_recover_masks (recover.hpp) runs.
//
// The prover (reference src/range/mod.rs:159-172 / :366-376, src/weighted_inner_product_proof.rs:94-95, :171, :175-227)
// starts from alpha_hat = alpha + y^(mn+1) S, S = gamma_0 for m = 1 (V_exp = y^(n+1), no z) and sum_j z^(2(j+1)) gamma_j
// for m > 1, adds e_t^2 d_L[t] + e_t^-2 d_R[t] in round t and ends with delta' = eta + delta e + alpha_k e^2.  With the
// challenge block [y, z, e, e_1..e_k] and the blinding slots [alpha, r, s, delta, eta, d_L[0..k), d_R[0..k)] known:
//     alpha_k = (delta' - eta - delta e) e^-2
//     S       = (alpha_k - sum_t (e_t^2 d_L[t] + e_t^-2 d_R[t]) - alpha) y^-(mn+1)
//     Gamma   = S for m = 1, S z^-2 for m > 1  =  gamma_0 + z^2 gamma_1 + .. + z^(2(m-1)) gamma_{m-1}
// As k + 2 independent terms: the k round terms, the final term (delta' - eta - delta e) e^-2 together with the scale
// (y^(mn+1) [z^2])^-1, and alpha.  A round term and the final term cost one inversion each.  A zero challenge leaves an
// inversion undefined: the term reports it and Gamma is written as zero.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "blind_layout.hpp"
#include "field.hpp"
#include "sha256.hpp"

namespace bpp {

// SHA-256 of ONE padded block from the initial state, in registers alone: w is the block (big-endian words) and is used up
// as the rolling message schedule.  sha::compress is one shared function whose state the caller keeps in memory; a value
// derived from a blinding key must not go there (on the device that memory is scratch).
BPP_HD void sha256_one_block(uint32_t w[16], uint32_t out[8]) {
    const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint32_t a = iv[0], b = iv[1], c = iv[2], d = iv[3], e = iv[4], f = iv[5], g = iv[6], hh = iv[7];
#pragma unroll
    for (int t = 0; t < 64; t++) {
        if (t >= 16) {
            const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
            const uint32_t s0 = sha::rotr(w15, 7) ^ sha::rotr(w15, 18) ^ (w15 >> 3);
            const uint32_t s1 = sha::rotr(w2, 17) ^ sha::rotr(w2, 19) ^ (w2 >> 10);
            w[t & 15] = w[t & 15] + s0 + w[(t + 9) & 15] + s1;
        }
        const uint32_t S1 = sha::rotr(e, 6) ^ sha::rotr(e, 11) ^ sha::rotr(e, 25);
        const uint32_t ch = (e & f) ^ (~e & g);
        const uint32_t t1 = hh + S1 + ch + sha::K256[t] + w[t & 15];
        const uint32_t S0 = sha::rotr(a, 2) ^ sha::rotr(a, 13) ^ sha::rotr(a, 22);
        const uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
        hh = g;
        g = f;
        f = e;
        e = d + t1;
        d = c;
        c = b;
        b = a;
        a = t1 + S0 + mj;
    }
    out[0] = iv[0] + a;
    out[1] = iv[1] + b;
    out[2] = iv[2] + c;
    out[3] = iv[3] + d;
    out[4] = iv[4] + e;
    out[5] = iv[5] + f;
    out[6] = iv[6] + g;
    out[7] = iv[7] + hh;
}
BPP_HD uint32_t bswap32(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }

// SHA-256(key || tag || idx as u64 LE || slot as u32 LE || h as u32 LE): the 52-byte block, one compression, that every
// value derived from a blinding key starts from -- a blinding slot here, the amount pad and the view tag in find_terms.hpp.
// key: 8 little-endian words; tag: the block's big-endian word, the domain separator; dg: the digest's big-endian words.
BPP_HD void key_block_digest(const uint32_t* key, uint32_t tag, uint64_t idx, uint32_t slot, uint32_t h, uint32_t dg[8]) {
    uint32_t w[16];
#pragma unroll
    for (int t = 0; t < 8; t++) w[t] = bswap32(key[t]);
    w[8] = tag;
    w[9] = bswap32((uint32_t)idx);
    w[10] = bswap32((uint32_t)(idx >> 32));
    w[11] = bswap32(slot);
    w[12] = bswap32(h);
    w[13] = 0x80000000u;
    w[14] = 0;
    w[15] = 52 * 8;
    sha256_one_block(w, dg);
}

// c_h = the digest of the block under "bppb", as 8 little-endian words of a 256-bit integer
BPP_HD void blind_half(const uint32_t* key, uint64_t idx, uint32_t slot, uint32_t h, uint32_t c[8]) {
    uint32_t dg[8];
    key_block_digest(key, bswap32(0x62707062u), idx, slot, h, dg);   // "bppb"
#pragma unroll
    for (int t = 0; t < 8; t++) c[t] = bswap32(dg[t]);
}

// Slot `slot` of the proof with blinding index idx under a 32-byte key (8 little-endian words): (c0 + 2^256 c1) mod r, zero
// replaced by one -- the value k_pb_blind (prover_batch.hpp) stores for the prover, here without a store: the recovery
// must leave nothing derived from the key in memory.  Pinned against each other by tests/test_recover_cpu.py (hashlib) and
// tests/test_gpu_recover.py (the device prover's proofs).
template <class P>
BPP_HD Fe<P> blind_slot(const uint32_t* key, uint64_t idx, uint32_t slot) {
    uint32_t c0[8], c1[8];
    blind_half(key, idx, slot, 0, c0);
    blind_half(key, idx, slot, 1, c1);
    uint32_t w128[8] = {0, 0, 0, 0, 1, 0, 0, 0};
    const Fe<P> f128 = fe_from_canonical<P>(w128);
    const Fe<P> f256 = fe_mul(f128, f128);
    Fe<P> x = fe_add(fe_from_canonical<P>(c0), fe_mul(fe_from_canonical<P>(c1), f256));
    if (x.is_zero()) x = Fe<P>::one();
    return x;
}

// the reference's literal blinding values the recovery needs (range/mod.rs:94 / :256; wip.rs:94-95, :177-178), one byte
// each in one word: alpha | d_L << 8 | d_R << 16 | delta << 24 | eta << 32.  A word and a shift, not five fields: a choice
// among fields is a choice among addresses to the compiler, and keeps the whole source below -- key included -- in memory.
BPP_HD uint64_t recover_literals(uint32_t alpha, uint32_t d_L, uint32_t d_R, uint32_t delta, uint32_t eta) {
    return (uint64_t)(alpha & 0xff) | (uint64_t)(d_L & 0xff) << 8 | (uint64_t)(d_R & 0xff) << 16 | (uint64_t)(delta & 0xff) << 24 |
           (uint64_t)(eta & 0xff) << 32;
}
// Where a proof's blinding scalars come from: have_key -- the slot expansion under key (held by value: a pointer to a
// kernel's argument block would make the compiler copy the block, key included, to memory) at index idx; else
// blind != null -- the proof's own 5 + 2k canonical scalars in the prover's layout; else the literals.
struct RecoverSource {
    bool have_key;
    uint32_t key[8];
    uint64_t idx;
    const uint32_t* blind;
    uint64_t lit;   // recover_literals
};
template <class P>
BPP_HD Fe<P> recover_slot(const RecoverSource& src, uint32_t k, uint32_t slot) {
    if (src.have_key) return blind_slot<P>(src.key, src.idx, slot);
    if (src.blind) {
        uint32_t w[8];
#pragma unroll
        for (int t = 0; t < 8; t++) w[t] = src.blind[(size_t)slot * 8 + t];
        return fe_from_canonical<P>(w);
    }
    const uint32_t at = slot == PB_BL_ALPHA ? 0u : slot == PB_BL_DELTA ? 24u : slot == PB_BL_ETA ? 32u : slot < PB_BL_DL + k ? 8u : 16u;
    const uint32_t lit = (uint32_t)(src.lit >> at) & 0xffu;
    return fe_from_u32<P>(lit);
}

// The terms of one proof.  Term t < k is round t, term k the final one, term k + 1 alpha.  Each is computed in three
// steps so that the lanes of a wave, which hold different terms, run ONE instruction stream through the expensive
// parts: the term's slots (recover_slot), the value x it has to invert (recover_*_x), the inversion, the term.
enum { RT_IDLE = 0, RT_ROUND, RT_FINAL, RT_ALPHA };
BPP_HD uint32_t recover_role(uint32_t t, uint32_t k) { return t < k ? RT_ROUND : t == k ? RT_FINAL : t == k + 1 ? RT_ALPHA : RT_IDLE; }
// the slots a term reads (b only for round and final terms)
BPP_HD uint32_t recover_slot_a(uint32_t role, uint32_t t) { return role == RT_ROUND ? PB_BL_DL + t : role == RT_FINAL ? PB_BL_DELTA : PB_BL_ALPHA; }
BPP_HD uint32_t recover_slot_b(uint32_t role, uint32_t t, uint32_t k) { return role == RT_ROUND ? PB_BL_DL + k + t : PB_BL_ETA; }

// round t: x = e_t^2
template <class P>
BPP_HD Fe<P> recover_round_x(const Fe<P>& e_t, bool& ok) {
    ok = !e_t.is_zero();
    return ok ? fe_sqr(e_t) : Fe<P>::one();
}
// - (e_t^2 d_L[t] + e_t^-2 d_R[t])
template <class P>
BPP_HD Fe<P> recover_round_term(const Fe<P>& dL, const Fe<P>& dR, const Fe<P>& x, const Fe<P>& xinv) {
    return fe_neg(fe_add(fe_mul(x, dL), fe_mul(xinv, dR)));
}
// final: x = e^2 den, den = y^(mn+1) (m = 1) or y^(mn+1) z^2 (m > 1); mn = 2^k
template <class P>
BPP_HD Fe<P> recover_final_x(const Fe<P>& y, const Fe<P>& z, const Fe<P>& e, uint32_t k, uint32_t m, Fe<P>& e2, Fe<P>& den,
                             bool& ok) {
    ok = !e.is_zero() && !y.is_zero() && (m == 1 || !z.is_zero());
    e2 = fe_sqr(e);
    den = y;
    for (uint32_t b = 0; b < k; b++) den = fe_sqr(den);
    den = fe_mul(den, y);
    if (m != 1) den = fe_mul(den, fe_sqr(z));
    return ok ? fe_mul(e2, den) : Fe<P>::one();
}
// (delta' - eta - delta e) e^-2, and the scale den^-1 the sum of all terms is multiplied by
template <class P>
BPP_HD Fe<P> recover_final_term(const Fe<P>& dprime, const Fe<P>& delta, const Fe<P>& eta, const Fe<P>& e, const Fe<P>& e2,
                                const Fe<P>& den, const Fe<P>& xinv, Fe<P>& scale) {
    scale = fe_mul(xinv, e2);
    return fe_mul(fe_sub(fe_sub(dprime, eta), fe_mul(delta, e)), fe_mul(xinv, den));
}

// Term t of a proof: its value (to be summed over t = 0 .. k + 1) and, from term k, the scale; ok false for a zero
// challenge.  triple: [r', s', delta'], ch: [y, z, e, e_1..e_k], canonical, 8 words each.
template <class P, class Inv>
BPP_HD Fe<P> recover_term(const RecoverSource& src, uint32_t k, uint32_t m, uint32_t t, const uint32_t* triple,
                          const uint32_t* ch, Fe<P>& scale, bool& ok, Inv&& inv) {
    using F = Fe<P>;
    const uint32_t role = recover_role(t, k);
    ok = true;
    F a = F::zero(), b = F::zero();
    if (role != RT_IDLE) a = recover_slot<P>(src, k, recover_slot_a(role, t));
    if (role == RT_ROUND || role == RT_FINAL) b = recover_slot<P>(src, k, recover_slot_b(role, t, k));
    F x = F::one(), e = F::zero(), e2 = F::zero(), den = F::zero();
    if (role == RT_ROUND) {
        x = recover_round_x(fe_from_canonical<P>(ch + (size_t)(3 + t) * 8), ok);
    } else if (role == RT_FINAL) {
        e = fe_from_canonical<P>(ch + 16);
        x = recover_final_x(fe_from_canonical<P>(ch), fe_from_canonical<P>(ch + 8), e, k, m, e2, den, ok);
    }
    const F xinv = inv(x);
    if (role == RT_ROUND) return recover_round_term(a, b, x, xinv);
    if (role == RT_FINAL) return recover_final_term(fe_from_canonical<P>(triple + 16), a, b, e, e2, den, xinv, scale);
    return role == RT_ALPHA ? fe_neg(a) : F::zero();
}

// Gamma of one proof, term after term: what the lanes of k_recover_masks compute side by side.  out: canonical words;
// zero (and false) for a zero challenge.
template <class P>
BPP_HD bool recover_mask(const RecoverSource& src, uint32_t k, uint32_t m, const uint32_t* triple, const uint32_t* ch,
                         uint32_t out[8]) {
    Fe<P> sum = Fe<P>::zero(), scale = Fe<P>::one();
    bool all_ok = true;
    for (uint32_t t = 0; t < k + 2; t++) {
        bool ok;
        Fe<P> sc = Fe<P>::one();
        sum = fe_add(sum, recover_term<P>(src, k, m, t, triple, ch, sc, ok, [](const Fe<P>& x) { return fe_inv(x); }));
        if (t == k) scale = sc;
        all_ok = all_ok && ok;
    }
    fe_to_canonical(all_ok ? fe_mul(sum, scale) : Fe<P>::zero(), out);
    return all_ok;
}

}  // namespace bpp
