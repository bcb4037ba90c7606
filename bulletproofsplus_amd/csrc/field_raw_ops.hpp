// field_raw_ops.hpp -- every operation of field.hpp behind one (op, a, b, c, d) -> out function on RAW limb images, for
// the tests alone.  Plain C++ beside field.hpp, so the debug kernel (tu_debug.hip, bpp_debug_field_raw_op) and the host
// build (tests/host/field_raw_host_test.cpp) compile the same text; tests/field_cases.py chooses the limbs -- all-ones
// limbs, values at 1, 2 and 8 p, unreduced sums -- and checks the result against Python integers.
//
// An operand is NL words, each a 30-bit limb, taken AS GIVEN: nothing is converted or reduced on the way in or out.
// The result is raw_out_words(NL) = 2 NL words, zero-filled behind what the operation writes:
//   an element            out[0 .. NL)
//   the _io forms         the product in out[0 .. NL), the operand as it was handed back in out[NL .. 2 NL)
//   a predicate           out[0] = 0 / 1
//   RAW_TO_CANONICAL      the N packed words in out[0 .. N)
//   RAW_STORE_LOAD        fe_load(fe_store(a)) in out[0 .. NL), the N stored words in out[NL .. NL + N)
// Scalar arguments ride in the operand words: RAW_POW_U64 takes its exponent from b[0] | b[1] << 32 (full words),
// RAW_FROM_U32 / RAW_FROM_I32 their argument from a[0] (a full word).
//
// The operations come in three groups, one kernel each on the device (the inverses carry loops and many registers that
// the short operations should not be compiled together with).
#pragma once
#include "field.hpp"

namespace bpp {

enum RawOp : int {
    // group 0: the multiplier
    RAW_MUL = 0,
    RAW_MUL_IO = 1,
    RAW_SQR = 2,
    RAW_SQR_IO = 3,
    RAW_MUL_ADD = 4,
    // group 1: sums, predicates, formats
    RAW_ADD = 5,
    RAW_SUB = 6,
    RAW_NEG = 7,
    RAW_DBL = 8,
    RAW_ADD_NR = 9,
    RAW_SUB_NR1 = 10,
    RAW_SUB_NR2 = 11,
    RAW_SUB_NR4 = 12,
    RAW_SUB_NR6 = 13,
    RAW_CSUB_NR4_POS = 14,
    RAW_CSUB_NR4_NEG = 15,
    RAW_ADD_DBL_NR = 16,
    RAW_IS_ZERO = 17,
    RAW_IS_ZERO_MOD5 = 18,
    RAW_EQ = 19,
    RAW_COND_SUB_P = 20,
    RAW_TO_CANONICAL = 21,
    RAW_STORE_LOAD = 22,
    RAW_FROM_U32 = 23,
    RAW_FROM_I32 = 24,
    // group 2: inverses and powers
    RAW_INV = 25,
    RAW_INV_PLAIN = 26,
    RAW_INV_FERMAT = 27,
    RAW_POW_U64 = 28,
    RAW_OP_COUNT = 29,
};

constexpr int RAW_GROUPS = 3;
constexpr int raw_op_group(int op) { return op < 0 || op >= RAW_OP_COUNT ? -1 : op <= RAW_MUL_ADD ? 0 : op <= RAW_FROM_I32 ? 1 : 2; }
constexpr int raw_out_words(int NL) { return 2 * NL; }

template <class P>
BPP_HD Fe<P> raw_limbs(const uint32_t* w) {
    Fe<P> r;
#pragma unroll
    for (int i = 0; i < P::NL; i++) r.l[i] = w[i];
    return r;
}
template <class P>
BPP_HD void raw_put(const Fe<P>& v, uint32_t* out) {
#pragma unroll
    for (int i = 0; i < P::NL; i++) out[i] = v.l[i];
}

// false: `op` is not an operation of group G
template <class P, int G>
BPP_HD bool fe_raw_op(int op, const uint32_t* wa, const uint32_t* wb, const uint32_t* wc, const uint32_t* wd, uint32_t* out) {
    constexpr int NL = P::NL, N = P::N;
    using F = Fe<P>;
    for (int i = 0; i < raw_out_words(NL); i++) out[i] = 0;
    F a = raw_limbs<P>(wa);
    const F b = raw_limbs<P>(wb);
    if constexpr (G == 0) {
        switch (op) {
            case RAW_MUL: raw_put(fe_mul(a, b), out); return true;
            case RAW_MUL_IO: {
                const F r = fe_mul_io(a, b);
                raw_put(r, out);
                raw_put(a, out + NL);
                return true;
            }
            case RAW_SQR: raw_put(fe_sqr(a), out); return true;
            case RAW_SQR_IO: {
                const F r = fe_sqr_io(a);
                raw_put(r, out);
                raw_put(a, out + NL);
                return true;
            }
            case RAW_MUL_ADD: raw_put(fe_mul_add(a, b, raw_limbs<P>(wc), raw_limbs<P>(wd)), out); return true;
            default: return false;
        }
    } else if constexpr (G == 1) {
        switch (op) {
            case RAW_ADD: raw_put(fe_add(a, b), out); return true;
            case RAW_SUB: raw_put(fe_sub(a, b), out); return true;
            case RAW_NEG: raw_put(fe_neg(a), out); return true;
            case RAW_DBL: raw_put(fe_dbl(a), out); return true;
            case RAW_ADD_NR: raw_put(fe_add_nr(a, b), out); return true;
            case RAW_SUB_NR1: raw_put(fe_sub_nr<1>(a, b), out); return true;
            case RAW_SUB_NR2: raw_put(fe_sub_nr<2>(a, b), out); return true;
            case RAW_SUB_NR4: raw_put(fe_sub_nr<4>(a, b), out); return true;
            case RAW_SUB_NR6: raw_put(fe_sub_nr<6>(a, b), out); return true;
            case RAW_CSUB_NR4_POS: raw_put(fe_csub_nr<4>(a, false, b), out); return true;
            case RAW_CSUB_NR4_NEG: raw_put(fe_csub_nr<4>(a, true, b), out); return true;
            case RAW_ADD_DBL_NR: raw_put(fe_add_dbl_nr(a, b), out); return true;
            case RAW_IS_ZERO: out[0] = a.is_zero() ? 1u : 0u; return true;
            case RAW_IS_ZERO_MOD5: out[0] = fe_is_zero_mod<5>(a) ? 1u : 0u; return true;
            case RAW_EQ: out[0] = a == b ? 1u : 0u; return true;
            case RAW_COND_SUB_P:
                fe_cond_sub_p(a);
                raw_put(a, out);
                return true;
            case RAW_TO_CANONICAL: {
                uint32_t w[N];
                fe_to_canonical(a, w);
                for (int i = 0; i < N; i++) out[i] = w[i];
                return true;
            }
            case RAW_STORE_LOAD: {
                uint32_t w[N];
                fe_store(a, w);
                raw_put(fe_load<P>(w), out);
                for (int i = 0; i < N; i++) out[NL + i] = w[i];
                return true;
            }
            case RAW_FROM_U32: raw_put(fe_from_u32<P>(wa[0]), out); return true;
            case RAW_FROM_I32: raw_put(fe_from_i32<P>((int32_t)wa[0]), out); return true;
            default: return false;
        }
    } else {
        static_assert(G == 2, "three groups");
        switch (op) {
            case RAW_INV: raw_put(fe_inv(a), out); return true;
            case RAW_INV_PLAIN: raw_put(fe_inv_plain(a), out); return true;
            case RAW_INV_FERMAT: raw_put(fe_inv_fermat(a), out); return true;
            case RAW_POW_U64: raw_put(fe_pow_u64(a, (uint64_t)wb[0] | ((uint64_t)wb[1] << 32)), out); return true;
            default: return false;
        }
    }
}

// the same with the group found from `op` (host builds; the device launches one kernel per group)
template <class P>
BPP_HD bool fe_raw_op_any(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out) {
    switch (raw_op_group(op)) {
        case 0: return fe_raw_op<P, 0>(op, a, b, c, d, out);
        case 1: return fe_raw_op<P, 1>(op, a, b, c, d, out);
        case 2: return fe_raw_op<P, 2>(op, a, b, c, d, out);
        default: return false;
    }
}

}  // namespace bpp
