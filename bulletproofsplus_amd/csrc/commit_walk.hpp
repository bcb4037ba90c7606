// commit_walk.hpp -- one commitment s g + gamma h as a walk over the window-table rows of generators 0 (g) and 1 (h) of an
// engine (kernels.hpp "window table"): RangeProver::commit, reference src/range/prover.rs:28-42, with the `v as i32` of
// prover.rs:37 or, in amount mode (BPP_PROVE_AMOUNT64), the whole u64.  Plain C++ beside ec.hpp and fixed_glv.hpp, so the
// host test (tests/host/commit_walk_host_test.cpp) compiles the very code k_commit_batch (commit.hpp) runs.
//
// The digits are those k_fixed_msm takes from the same tables (fixed_glv.hpp win_biased / win_next_digit), of the whole
// scalar or, on BLS12-381, of the halves of its endomorphism split (glv_split_balanced): there the walk sums both k2
// halves negated, multiplies the accumulator's X by beta once and adds both k1 halves.  A non-zero digit is
// one table entry and one lazy mixed addition; a zero digit is nothing, so a 64-bit amount costs at most
// ceil(65 / c) additions on g whatever the scalar field's width.  xyzz_madd_lazy is complete (P + P, P - P): with the
// reference's test key h = 2 g both occur.
#pragma once
#include <cstddef>
#include <cstdint>

#include "ed25519.hpp"
#include "fixed_glv.hpp"

namespace bpp {

// the table serves the two halves of the endomorphism split (kernels.hpp fixed_glv<C>())
template <class C>
constexpr bool commit_walk_glv() {
    return C::ID == 0;
}

// canonical words of the scalar on g: the amount itself, or PrimeFieldElem::new(v as i32) (negative: r - |v|)
template <class C>
BPP_HD void commit_amount_scalar(uint64_t v, bool amount64, uint32_t out[8]) {
    using P = typename C::Fr;
#pragma unroll
    for (int t = 0; t < 8; t++) out[t] = 0;
    if (amount64) {
        out[0] = (uint32_t)v;
        out[1] = (uint32_t)(v >> 32);
        return;
    }
    const int32_t vi = (int32_t)(uint32_t)v;
    if (vi >= 0)
        out[0] = (uint32_t)vi;
    else
        fe_to_canonical(fe_from_i32<P>(vi), out);
}

// S: the window layout (VerifyShape, or a WinLayout): W, per_f, bias[], wc[], went[].  kv, kg: canonical scalars (< r) on g
// and h.  load_entry(e) -> Aff<C>: entry e of the table (generator f's row starts at f * per_f).  add(acc, entry, neg):
// acc += neg ? -entry : entry.
template <class C, class S, class Load, class Add>
BPP_HD Xyzz<C> commit_walk(const S& s, const uint32_t kv[8], const uint32_t kg[8], Load&& load_entry, Add&& add) {
    constexpr bool GLV = commit_walk_glv<C>();
    constexpr int NW = GLV ? GLV_HALF_WORDS : WIN_FULL_WORDS;
    Xyzz<C> acc = xyzz_inf<C>();
    // the digit loop: the value k (a scalar, or a half that stands for its negative if hneg) over generator f's row
    auto walk = [&](const uint32_t* k, uint32_t f, bool hneg) {
        uint32_t w[NW];
        win_biased<NW>(k, s.bias, w);
        for (uint32_t j = 0; j < s.W; j++) {
            const int32_t dg = win_next_digit(w, win_width(s, j));   // width 0: the top window
            if (dg == 0) continue;
            const uint32_t mag = dg < 0 ? (uint32_t)(-dg) : (uint32_t)dg;
            add(acc, load_entry((size_t)f * s.per_f + s.went[j] + (mag - 1)), (dg < 0) != hneg);
        }
    };
    if constexpr (GLV) {
        // the four halves stay in registers: they are chosen by selects on the (wave-uniform) step, never indexed
        uint32_t k1v[4], k2v[4], k1g[4], k2g[4];
        bool n1v, n2v, n1g, n2g;
        glv_split_balanced<C>(kv, k1v, k2v, n1v, n2v);
        glv_split_balanced<C>(kg, k1g, k2g, n1g, n2g);
#pragma unroll 1
        for (uint32_t step = 0; step < 4; step++) {   // k2 of v, k2 of gamma, then k1 of v, k1 of gamma
            const bool phase = step >= 2;
            const uint32_t f = step & 1u;
            if (step == 2) xyzz_mul_x_beta(acc);   // [z^2] of the k2 sum, summed negated: psi(-S) = (beta X, Y)
            uint32_t h[4];
#pragma unroll
            for (int t = 0; t < 4; t++) h[t] = phase ? (f ? k1g[t] : k1v[t]) : (f ? k2g[t] : k2v[t]);
            walk(h, f, phase ? (f ? n1g : n1v) : !(f ? n2g : n2v));
        }
    } else {
#pragma unroll 1
        for (uint32_t f = 0; f < 2; f++) {
            uint32_t k[8];   // chosen by selects, as the halves are: an indexed scalar would go to scratch
#pragma unroll
            for (int t = 0; t < 8; t++) k[t] = f ? kg[t] : kv[t];
            walk(k, f, false);
        }
    }
    return acc;
}

}  // namespace bpp
