// recover_coeffs.hpp -- mask recovery for MANY keys: what of recover_terms.hpp's formula does not depend on the key.
// Plain C++ beside recover_terms.hpp, so the host test (tests/host/recover_keys_host_test.cpp) compiles the very code
// k_recover_coeffs, k_scan_keys and k_scan_keys_confirm (recover_keys.hpp) run.
//
// Gamma is affine in the blinding slots [alpha, r, s, delta, eta, d_L[0..k), d_R[0..k)] of a proof, and the coefficients
// are public functions of its challenge block [y, z, e, e_1..e_k] and of delta' (recover_terms.hpp multiplied out):
//     Gamma = A0 + sum_s c_s slot_s(key, index)
//     c_alpha = -D   c_delta = -D e^-1   c_eta = -D e^-2   c_dL[t] = -D e_t^2   c_dR[t] = -D e_t^-2   c_r = c_s = 0
//     A0 = D e^-2 delta'      D = (y^(nm+1))^-1 for m = 1, (y^(nm+1) z^2)^-1 for m > 1
// so a scan under K keys inverts once per proof (the k + 1 inversions of recover_terms.hpp) and spends 2k + 3 slot
// expansions and as many products per (key, proof) pair.  The inverted values are recover_round_x / recover_final_x of
// recover_terms.hpp: a zero challenge is undefined here exactly where it is there.
//
// Also here: the comparison of a commitment walk's accumulator with a decoded wire point WITHOUT the inversion of
// jac_to_aff (walk_equals_wire), for the confirmation of a pair.
#pragma once
#include "commit_walk.hpp"
#include "recover_terms.hpp"
#include "ristretto.hpp"

namespace bpp {

// The slots that carry a non-zero coefficient, numbered 0 .. 2k + 2: alpha, delta, eta, d_L[0..k), d_R[0..k).
BPP_HD uint32_t coeff_live_slots(uint32_t k) { return 2 * k + 3; }
BPP_HD uint32_t coeff_live_slot(uint32_t l) { return l ? l + 2 : (uint32_t)PB_BL_ALPHA; }
// A proof's coefficients as the kernels keep them: [A0, c of live slot 0, 1, ..], 2k + 4 field elements
BPP_HD uint32_t coeff_elems(uint32_t k) { return 2 * k + 4; }

// Term t of a proof (recover_role: t < k round t, t = k the final term) names the value x it has to invert; ok false for
// a zero challenge (then x = 1).  Term k also hands back e, e^2 and den = y^(nm+1) [z^2].
template <class P>
BPP_HD Fe<P> coeff_term_x(uint32_t k, uint32_t m, uint32_t t, const uint32_t* ch, Fe<P>& e, Fe<P>& e2, Fe<P>& den, bool& ok) {
    using F = Fe<P>;
    const uint32_t role = recover_role(t, k);
    ok = true;
    F x = F::one();
    if (role == RT_ROUND) {
        x = recover_round_x(fe_from_canonical<P>(ch + (size_t)(3 + t) * 8), ok);
    } else if (role == RT_FINAL) {
        e = fe_from_canonical<P>(ch + 16);
        x = recover_final_x(fe_from_canonical<P>(ch), fe_from_canonical<P>(ch + 8), e, k, m, e2, den, ok);
    }
    return x;
}
// the final term, from xinv = (e^2 den)^-1: D = den^-1 and head = [A0, c_alpha, c_delta, c_eta]
template <class P>
BPP_HD void coeff_head(const Fe<P>& dprime, const Fe<P>& e, const Fe<P>& e2, const Fe<P>& den, const Fe<P>& xinv, Fe<P>& D,
                       Fe<P> head[4]) {
    D = fe_mul(xinv, e2);
    const Fe<P> einv2 = fe_mul(xinv, den);
    head[1] = fe_neg(D);
    head[3] = fe_mul(head[1], einv2);
    head[2] = fe_mul(head[3], e);
    head[0] = fe_mul(fe_mul(D, einv2), dprime);
}
// round t, from x = e_t^2 and its inverse
template <class P>
BPP_HD void coeff_round(const Fe<P>& D, const Fe<P>& x, const Fe<P>& xinv, Fe<P>& c_dL, Fe<P>& c_dR) {
    const Fe<P> nD = fe_neg(D);
    c_dL = fe_mul(nD, x);
    c_dR = fe_mul(nD, xinv);
}

// All coefficients of one proof, term after term: what the lanes of k_recover_coeffs compute side by side.
// out[slot] for the 5 + 2k slots of blind_layout.hpp (out[r] = out[s] = 0), out[5 + 2k] = A0.  ok false for a zero
// challenge (out is then not meaningful).  triple: [r', s', delta'], ch: [y, z, e, e_1..e_k], canonical words.
template <class P>
BPP_HD void recover_coeffs(uint32_t k, uint32_t m, const uint32_t* triple, const uint32_t* ch, Fe<P>* out, bool& ok) {
    using F = Fe<P>;
    F e = F::zero(), e2 = F::zero(), den = F::zero(), D, head[4];
    bool okt;
    const F xf = coeff_term_x<P>(k, m, k, ch, e, e2, den, okt);
    ok = okt;
    coeff_head(fe_from_canonical<P>(triple + 16), e, e2, den, fe_inv(xf), D, head);
    out[PB_BL_ALPHA] = head[1];
    out[PB_BL_R] = F::zero();
    out[PB_BL_S] = F::zero();
    out[PB_BL_DELTA] = head[2];
    out[PB_BL_ETA] = head[3];
    out[pb_blind_elems(k)] = head[0];
    for (uint32_t t = 0; t < k; t++) {
        F u0, u1, u2;
        const F x = coeff_term_x<P>(k, m, t, ch, u0, u1, u2, okt);
        ok = ok && okt;
        coeff_round(D, x, fe_inv(x), out[PB_BL_DL + t], out[PB_BL_DL + k + t]);
    }
}

// One live slot's share of Gamma under a key: c slot(key, idx).  The slot expansion is blind_slot's, in registers.
template <class P>
BPP_HD Fe<P> coeff_slot_share(const uint32_t* key, uint64_t idx, uint32_t slot, const Fe<P>& c) {
    return fe_mul(blind_slot<P>(key, idx, slot), c);
}

// Is the accumulator of a commitment walk the point a decoded record holds (V: wire words x | y | inf)?  The answer of
// aff_to_wire(jac_to_aff(xyzz_to_jac(acc))) compared with V as k_recover_confirm compares them, without the inversion:
// Weierstrass X == x ZZ and Y == y ZZZ with the infinity flags (the walk leaves X < 6p, Y <= 2p: a product with one brings
// both below 2p, where == is exact); edwards25519 the relation rist_equal tests, X y == Y x || Y y == X x on the
// accumulator's coordinates -- the common Z cancels, and the identity's wire image decodes to (0, 1) as it does there.
template <class C>
BPP_HD bool walk_equals_wire(const Xyzz<C>& acc, const uint32_t* V) {
    using F = Fe<typename C::Fp>;
    constexpr int N = C::Fp::N;
    const bool inf_V = (V[2 * N] | V[2 * N + 1]) != 0;
    if constexpr (C::ID == 2) {
        Aff<C> b = aff_inf<C>();
        if (!inf_V) {
            b.x = fe_from_canonical<typename C::Fp>(V);
            b.y = fe_from_canonical<typename C::Fp>(V + N);
        }
        const Jac<C> a = xyzz_to_jac(acc);
        return fe_mul(a.X, b.y) == fe_mul(a.Y, b.x) || fe_mul(a.Y, b.y) == fe_mul(a.X, b.x);
    } else {
        if (acc.is_inf() || inf_V) return acc.is_inf() && inf_V;
        const F x = fe_from_canonical<typename C::Fp>(V), y = fe_from_canonical<typename C::Fp>(V + N);
        return fe_mul(acc.X, F::one()) == fe_mul(x, acc.ZZ) && fe_mul(acc.Y, F::one()) == fe_mul(y, acc.ZZZ);
    }
}

}  // namespace bpp
