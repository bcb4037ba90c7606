// tu_debug.hip -- the device-side unit-test hooks: the field and group primitives on canonical values
// (bpp_debug_field_op / bpp_debug_point_op), and on RAW register images the field operations at limbs the test chooses
// (field_raw_ops.hpp), the lazy mixed addition on a raw accumulator, and the scalar splits / digit recoding as the
// device compiles them.  A translation unit of its own: none of this is compiled into the units of the hot kernels.
// The entries are not part of include/bpp_amd.h.
// Every pointer is a host pointer -- except in bpp_debug_verifier_mulvec, the verifier's back end (VerifyImpl::run_stage) on
// MulVec scalars the test chooses, which takes device buffers as bpp_verifier_run does and adds no kernel.  Its front half,
// the scalar stage (launch_verify_scalars) on challenges the test chooses, is bpp_debug_verifier_scalars: host pointers again.
// bpp_debug_scan_keys is that hook's counterpart for the many-key scan (recover_keys.hpp): a class of chosen proofs through
// k_recover_coeffs and k_scan_keys, host pointers, no kernel of its own.  bpp_debug_prover_scalars is the batched prover's:
// k_pb_init, k_pb_round and k_pb_final whole, on witnesses, blinding and challenges the test chooses, through
// ProveBatchImpl::prove_batch_device -- host pointers, no kernel of its own.  bpp_debug_verifier_table reads the verifier's
// window tables back entry by entry, raw and through k_points_to_wire (VerifyImpl::table_slice) -- host pointers, no kernel
// of its own.
#include "host_util.hpp"

#include "field_raw_ops.hpp"
#include "fixed_glv.hpp"
#include "impl_prove_batch.hpp"   // declarations only: the kernels of prover_batch.hpp live in tu_prove_*.hip
#include "impl_verify.hpp"   // declarations only (no BPP_IMPL_DEFINITIONS): the kernels live in tu_verify_*.hip
#include "recover_keys.hpp"  // likewise: k_recover_coeffs and k_scan_keys live in tu_recover_keys_*.hip

namespace bpp {

template <class P>
__global__ void __launch_bounds__(64) k_dbg_field(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t wa[P::N], wb[P::N], wr[P::N];
    for (int t = 0; t < P::N; t++) {
        wa[t] = a[i * P::N + t];
        wb[t] = b[i * P::N + t];
    }
    Fe<P> x = fe_from_canonical<P>(wa), y = fe_from_canonical<P>(wb), r;
    switch (op) {
        case 0: r = fe_mul(x, y); break;
        case 1: r = fe_add(x, y); break;
        case 2: r = fe_sub(x, y); break;
        case 3: r = fe_inv(x); break;
        case 4: r = fe_sqr(x); break;
        default: r = fe_neg(x); break;
    }
    fe_to_canonical(r, wr);
    for (int t = 0; t < P::N; t++) out[i * P::N + t] = wr[t];
}

template <class C>
__global__ void __launch_bounds__(64) k_dbg_point(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
    constexpr int WW = 2 * C::Fp::N + 2;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t wa[WW], wb[WW], wr[WW];
    for (int t = 0; t < WW; t++) {
        wa[t] = a[i * WW + t];
        wb[t] = b[i * WW + t];
    }
    Aff<C> p, q;
    aff_from_wire<C>(wa, p);
    aff_from_wire<C>(wb, q);
    Jac<C> r;
    switch (op) {
        case 0: r = jac_add(jac_from_aff(p), jac_from_aff(q)); break;
        case 1: r = jac_madd(jac_from_aff(p), q); break;
        case 2: r = jac_dbl(jac_from_aff(p)); break;
        case 3: r = jac_madd(jac_dbl(jac_from_aff(p)), q); break;  // non-trivial Z
        case 4: r = jac_add(jac_dbl(jac_from_aff(p)), jac_dbl(jac_from_aff(q))); break;
        default: {  // XYZZ accumulator: inf + p + q + p
            Xyzz<C> acc = xyzz_inf<C>();
            acc = xyzz_madd(acc, p);
            acc = xyzz_madd(acc, q);
            acc = xyzz_madd(acc, p);
            r = xyzz_to_jac(acc);
            break;
        }
    }
    aff_to_wire(jac_to_aff(r), wr);
    for (int t = 0; t < WW; t++) out[i * WW + t] = wr[t];
}

template <class P, int G>
__global__ void __launch_bounds__(64) k_dbg_field_raw(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                                       const uint32_t* d, uint32_t* out, uint32_t* bad, size_t n) {
    constexpr int NL = P::NL, OW = raw_out_words(NL);
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t wa[NL], wb[NL], wc[NL], wd[NL], wr[OW];
    for (int t = 0; t < NL; t++) {
        wa[t] = a[i * NL + t];
        wb[t] = b[i * NL + t];
        wc[t] = c[i * NL + t];
        wd[t] = d[i * NL + t];
    }
    if (!fe_raw_op<P, G>(op, wa, wb, wc, wd, wr)) *bad = 1u;
    for (int t = 0; t < OW; t++) out[i * OW + t] = wr[t];
}

// acc: 4 raw elements (X | Y | ZZ | ZZZ, on edwards25519 X | Y | Z | T); q: 2 raw elements, canonical (x, y < p)
template <class C>
__global__ void __launch_bounds__(64) k_dbg_madd_lazy_raw(const uint32_t* acc, const uint32_t* q, const uint32_t* neg,
                                                           uint32_t* out, size_t n) {
    using P = typename C::Fp;
    constexpr int NL = P::NL;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fe<P> e[4];
    for (int t = 0; t < 4; t++) e[t] = raw_limbs<P>(acc + (i * 4 + t) * NL);
    Aff<C> pt;
    pt.x = raw_limbs<P>(q + (i * 2) * NL);
    pt.y = raw_limbs<P>(q + (i * 2 + 1) * NL);
    Xyzz<C> p;
    if constexpr (C::ID == 2) {
        p.e.X = e[0], p.e.Y = e[1], p.e.Z = e[2], p.e.T = e[3];
    } else {
        p.X = e[0], p.Y = e[1], p.ZZ = e[2], p.ZZZ = e[3];
    }
    xyzz_madd_lazy(p, pt, neg[i] != 0);
    if constexpr (C::ID == 2) {
        e[0] = p.e.X, e[1] = p.e.Y, e[2] = p.e.Z, e[3] = p.e.T;
    } else {
        e[0] = p.X, e[1] = p.Y, e[2] = p.ZZ, e[3] = p.ZZZ;
    }
    for (int t = 0; t < 4; t++) raw_put(e[t], out + (i * 4 + t) * NL);
}

constexpr int GLV_SPLIT_OUT = 10;   // k1[4] | k2[4] | neg1 | neg2

// op 0 glv_split, 1 glv_split_balanced, 2 glv_split_signed: k = 8 canonical words per scalar
template <class C>
__global__ void __launch_bounds__(64) k_dbg_glv_split(int op, const uint32_t* k, uint32_t* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t kk[8], k1[4], k2[4];
    for (int t = 0; t < 8; t++) kk[t] = k[i * 8 + t];
    bool n1 = false, n2 = false;
    if constexpr (C::ID == 0) {
        if (op == 0) glv_split<C>(kk, k1, k2);
        else if (op == 1) glv_split_balanced<C>(kk, k1, k2, n1, n2);
        else glv_split_signed<C>(kk, k1, k2, n1, n2);
    } else {
        glv_split_signed<C>(kk, k1, k2, n1, n2);
    }
    for (int t = 0; t < 4; t++) {
        out[i * GLV_SPLIT_OUT + t] = k1[t];
        out[i * GLV_SPLIT_OUT + 4 + t] = k2[t];
    }
    out[i * GLV_SPLIT_OUT + 8] = n1 ? 1u : 0u;
    out[i * GLV_SPLIT_OUT + 9] = n2 ? 1u : 0u;
}

// op 3: values of NK words (4: a half, NW = 5; 8: a whole scalar, NW = 10) -> the L.W digits of win_biased /
// win_next_digit, ROW words per value
constexpr int GLV_RECODE_ROW = 64;   // the split layout's rows: a half never has more windows
template <int NW, int ROW>
__global__ void __launch_bounds__(64) k_dbg_win_recode(WinLayout L, const uint32_t* k, uint32_t* out, size_t n) {
    constexpr int NK = NW == GLV_HALF_WORDS ? 4 : 8;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t kk[NK], v[NW];
    for (int t = 0; t < NK; t++) kk[t] = k[i * NK + t];
    win_biased<NW>(kk, L.bias, v);
    for (uint32_t j = 0; j < (uint32_t)ROW; j++) out[i * ROW + j] = j < L.W ? (uint32_t)win_next_digit(v, win_width(L, j)) : 0u;
}

template <class F>
static int on_ctx_device(const bpp_ctx* ctx, size_t n, F&& f) noexcept {
    return guarded(Count{n, "n"}, [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        return dispatch(ctx->curve, f);
    });
}

template <class P>
static int field_raw_op(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, size_t n, uint32_t* out) {
    const size_t in_bytes = n * P::NL * 4, out_bytes = n * raw_out_words(P::NL) * 4;
    DevBuf da, db, dc, dd, dout, dbad;
    HIPCHK(da.upload(a, in_bytes));
    HIPCHK(db.upload(b, in_bytes));
    HIPCHK(dc.upload(c, in_bytes));
    HIPCHK(dd.upload(d, in_bytes));
    HIPCHK(dout.alloc(out_bytes));
    HIPCHK(dbad.alloc(4));
    HIPCHK(hipMemset(dbad.p, 0, 4));
    if (n) {
        const dim3 grid(cdiv(n, 64)), block(64);
        switch (raw_op_group(op)) {
            case 0: hipLaunchKernelGGL((k_dbg_field_raw<P, 0>), grid, block, 0, nullptr, op, da.u32(), db.u32(), dc.u32(), dd.u32(), dout.u32(), dbad.u32(), n); break;
            case 1: hipLaunchKernelGGL((k_dbg_field_raw<P, 1>), grid, block, 0, nullptr, op, da.u32(), db.u32(), dc.u32(), dd.u32(), dout.u32(), dbad.u32(), n); break;
            case 2: hipLaunchKernelGGL((k_dbg_field_raw<P, 2>), grid, block, 0, nullptr, op, da.u32(), db.u32(), dc.u32(), dd.u32(), dout.u32(), dbad.u32(), n); break;
            default: return fail(BPP_E_ARG, "unknown raw field op");
        }
        HIPCHK(hipGetLastError());
    }
    uint32_t bad = 0;
    HIPCHK(dbad.download(&bad, 4));
    if (bad) return fail(BPP_E_ARG, "unknown raw field op");
    if (out_bytes) HIPCHK(dout.download(out, out_bytes));
    return BPP_OK;
}

// field: 0 = base field, 1 = scalar field; a, b, out: n elements of P::N canonical words
template <class P>
static int field_op(int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out) {
    DevBuf da, db, dout;
    const size_t bytes = n * P::N * 4;
    HIPCHK(da.upload(a, bytes));
    HIPCHK(db.upload(b, bytes));
    HIPCHK(dout.alloc(bytes));
    hipLaunchKernelGGL(k_dbg_field<P>, dim3(cdiv(n, 64)), dim3(64), 0, nullptr, op, da.u32(), db.u32(), dout.u32(), n);
    HIPCHK(hipGetLastError());
    HIPCHK(dout.download(out, bytes));
    return BPP_OK;
}

template <class C>
static int point_op(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
    DevBuf da, db, dout;
    const size_t bytes = n * wire_words<C>() * 4;
    HIPCHK(da.upload(a, bytes));
    HIPCHK(db.upload(b, bytes));
    HIPCHK(dout.alloc(bytes));
    hipLaunchKernelGGL(k_dbg_point<C>, dim3(cdiv(n, 64)), dim3(64), 0, nullptr, op, da.u32(), db.u32(), dout.u32(), n);
    HIPCHK(hipGetLastError());
    HIPCHK(dout.download(out, bytes));
    return BPP_OK;
}

}  // namespace bpp

using namespace bpp;

// The field and group primitives on canonical values (tests/ check them against a CPU checker).
// field: 0 = base field, 1 = scalar field; op: 0 mul, 1 add, 2 sub, 3 inv, 4 sqr, 5 neg
// a, b, out: n elements of N 32-bit words (N = 12 for BLS12-381 Fp, else 8), host pointers
extern "C" int bpp_debug_field_op(bpp_ctx* ctx, int field, int op, const uint32_t* a, const uint32_t* b, size_t n,
                                  uint32_t* out) {
    if (!ctx || !a || !b || !out) return fail(BPP_E_ARG, "null argument");
    return on_ctx_device(ctx, n, [&](auto cv) -> int {
        using C = decltype(cv);
        if (field == 0) return field_op<typename C::Fp>(op, a, b, n, out);
        return field_op<typename C::Fr>(op, a, b, n, out);
    });
}
// op: 0 add, 1 madd, 2 dbl(a), 3 madd(2a, b), 4 add(2a, 2b), 5 xyzz: inf + a + b + a; wire points, host pointers
extern "C" int bpp_debug_point_op(bpp_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, size_t n,
                                  uint64_t* out) {
    if (!ctx || !a || !b || !out) return fail(BPP_E_ARG, "null argument");
    return on_ctx_device(ctx, n, [&](auto cv) -> int { return point_op<decltype(cv)>(op, a, b, n, out); });
}

// field: 0 = base field, 1 = scalar field; op: a RawOp of field_raw_ops.hpp.  a, b, c, d: n operands of NL words each
// (30-bit limbs, taken as given; every operation reads only the operands it has, but all four must be readable);
// out: n results of 2 NL words.
extern "C" int bpp_debug_field_raw_op(bpp_ctx* ctx, int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                      const uint32_t* d, size_t n, uint32_t* out) {
    if (!ctx || !a || !b || !c || !d || !out) return fail(BPP_E_ARG, "null argument");
    if (raw_op_group(op) < 0) return fail(BPP_E_ARG, "unknown raw field op");
    return on_ctx_device(ctx, n, [&](auto cv) -> int {
        using C = decltype(cv);
        if (field == 0) return field_raw_op<typename C::Fp>(op, a, b, c, d, n, out);
        return field_raw_op<typename C::Fr>(op, a, b, c, d, n, out);
    });
}

// xyzz_madd_lazy(acc, q, neg) on n raw accumulators: acc 4 NL words each (X | Y | ZZ | ZZZ; edwards25519: X | Y | Z | T),
// q 2 NL words each (Montgomery form, canonical), neg one word each; out: the accumulators afterwards, 4 NL words each.
extern "C" int bpp_debug_madd_lazy_raw(bpp_ctx* ctx, const uint32_t* acc, const uint32_t* q, const uint32_t* neg, size_t n,
                                       uint32_t* out) {
    if (!ctx || !acc || !q || !neg || !out) return fail(BPP_E_ARG, "null argument");
    return on_ctx_device(ctx, n, [&](auto cv) -> int {
        using C = decltype(cv);
        constexpr int NL = C::Fp::NL;
        DevBuf dacc, dq, dneg, dout;
        HIPCHK(dacc.upload(acc, n * 4 * NL * 4));
        HIPCHK(dq.upload(q, n * 2 * NL * 4));
        HIPCHK(dneg.upload(neg, n * 4));
        HIPCHK(dout.alloc(n * 4 * NL * 4));
        if (n) {
            hipLaunchKernelGGL(k_dbg_madd_lazy_raw<C>, dim3(cdiv(n, 64)), dim3(64), 0, nullptr, dacc.u32(), dq.u32(), dneg.u32(),
                               dout.u32(), n);
            HIPCHK(hipGetLastError());
            HIPCHK(dout.download(out, n * 4 * NL * 4));
        }
        return BPP_OK;
    });
}

// The scalar splits and the digit recoding of the fixed-generator tables, from a kernel.
//   op 0 glv_split, 1 glv_split_balanced (BLS12-381), 2 glv_split_signed (BLS12-381, secp256k1): in = n scalars of 8
//     canonical words; out = 10 words each: k1[4] | k2[4] | neg1 | neg2.
//   op 3 win_biased + win_next_digit for the layout of window_bits (every curve; fixed_glv.hpp).  BLS12-381: in = n
//     halves of 4 words, ROW = 64; secp256k1, edwards25519: in = n scalars of 8 canonical words, ROW = 128 (VS_MAXW).
//     out = ROW words each, the W digits (two's complement) then zeros; out_layout (may be null) = W | top | per_f | ROW
//     window widths.
extern "C" int bpp_debug_glv_op(bpp_ctx* ctx, int op, int window_bits, const uint32_t* in, size_t n, uint32_t* out,
                                uint32_t* out_layout) {
    if (!ctx || !in || !out) return fail(BPP_E_ARG, "null argument");
    if (op < 0 || op > 3) return fail(BPP_E_ARG, "unknown glv op");
    if (op == 3 && (window_bits < 2 || window_bits > 20)) return fail(BPP_E_ARG, "window_bits must be in [2, 20]");
    return on_ctx_device(ctx, n, [&](auto cv) -> int {
        using C = decltype(cv);
        if (op == 3) {
            constexpr bool GLV = fixed_glv<C>();
            constexpr int NW = GLV ? GLV_HALF_WORDS : WIN_FULL_WORDS, ROW = GLV ? GLV_RECODE_ROW : VS_MAXW;
            WinLayout L;
            bool have;
            if constexpr (GLV) {
                uint32_t hmax[4];
                glv_half_max<C>(hmax);
                have = glv_layout(window_bits, C::Fr::BITS, hmax, L);
            } else {
                have = !win_layout_uniform(window_bits, C::Fr::MODW, C::Fr::BITS, L);
            }
            if (!have || L.W > (uint32_t)ROW) return fail(BPP_E_ARG, "no layout at this window_bits");
            if (out_layout) {
                out_layout[0] = L.W, out_layout[1] = L.top, out_layout[2] = L.per_f;
                for (int j = 0; j < ROW; j++) out_layout[3 + j] = L.wc[j];
            }
            DevBuf din, dout;
            HIPCHK(din.upload(in, n * (GLV ? 4 : 8) * 4));
            HIPCHK(dout.alloc(n * ROW * 4));
            if (n) {
                hipLaunchKernelGGL((k_dbg_win_recode<NW, ROW>), dim3(cdiv(n, 64)), dim3(64), 0, nullptr, L, din.u32(), dout.u32(), n);
                HIPCHK(hipGetLastError());
                HIPCHK(dout.download(out, n * ROW * 4));
            }
            return BPP_OK;
        } else if constexpr (!curve_has_glv<C>()) {
            return fail(BPP_E_ARG, "this curve has no scalar split");
        } else {
            if (op != 2 && C::ID != 0) return fail(BPP_E_ARG, "BLS12-381 only");
            DevBuf din, dout;
            HIPCHK(din.upload(in, n * 8 * 4));
            HIPCHK(dout.alloc(n * GLV_SPLIT_OUT * 4));
            if (n) {
                hipLaunchKernelGGL(k_dbg_glv_split<C>, dim3(cdiv(n, 64)), dim3(64), 0, nullptr, op, din.u32(), dout.u32(), n);
                HIPCHK(hipGetLastError());
                HIPCHK(dout.download(out, n * GLV_SPLIT_OUT * 4));
            }
            return BPP_OK;
        }
    });
}

// m_view -> the class whose shape VerifyImpl::class_shape returns (beyond every view: the verifier's own shape)
static bool debug_view_shape(const bpp_verifier* v, uint32_t m_view, uint32_t& cls) {
    if (m_view == 0) {
        cls = (uint32_t)MIXED_CLASSES;
        return true;
    }
    if ((m_view & (m_view - 1)) || m_view >= v->s.m) return false;
    for (cls = 0; (1u << cls) < m_view; cls++) {}
    return true;
}

// The verifier's scalar stage -- k_vs_prepare and k_vs_expand through launch_verify_scalars, the function every pass calls
// (with its dynamic-LDS opt-in) -- on proof scalars and challenges the caller chooses.  Host pointers, synchronous.
//   m_view: as for bpp_debug_verifier_mulvec below; N and k are that shape's.
//   scalars3 [count][3][4]: r', s', delta' ; challenges [count][3 + k][4]: y, z, e, e_1..e_k per proof (any 256-bit words:
//     the kernels reduce them), or null: the shape's literals for every proof ; out [count][N][4]: the MulVec's scalars.
extern "C" int bpp_debug_verifier_scalars(bpp_verifier* v, uint32_t m_view, const uint64_t* scalars3, const uint64_t* challenges,
                                          size_t count, uint64_t* out) {
    if (!v || !scalars3 || !out) return fail(BPP_E_ARG, "null argument");
    uint32_t cls = 0;
    if (!debug_view_shape(v, m_view, cls)) return fail(BPP_E_ARG, "m_view must be 0 or a power of two below m");
    if (count == 0) return BPP_OK;
    if (count > 0x7fffffffu / 64) return fail(BPP_E_ARG, "count too large for one launch");
    return guarded(Count{count, "count"}, [&]() -> int {
        HIPCHK(hipSetDevice(v->ctx.device));
        return dispatch(v->ctx.curve, [&](auto cv) -> int {
            using C = decltype(cv);
            const VerifyShape s = VerifyImpl<C>::class_shape(v, cls).s;
            const size_t ch_words = (size_t)(3 + s.k) * 8, out_bytes = count * (size_t)s.N * 32;
            DevBuf dps, dch, dprep, dout;
            HIPCHK(dps.upload(scalars3, count * 96));
            if (challenges) {
                HIPCHK(dch.upload(challenges, count * ch_words * 4));
            } else {
                std::vector<uint32_t> lit;
                default_challenges(s, lit);
                HIPCHK(dch.upload(lit.data(), lit.size() * 4));
            }
            HIPCHK(dprep.alloc(count * vs_prep_bytes<C>(s)));
            HIPCHK(dout.alloc(out_bytes));
            if (int rc = launch_verify_scalars<C>(s, dps.u32(), dch.u32(), challenges ? (uint32_t)ch_words : 0u, dout.u32(), count,
                                                  dprep.u32(), nullptr))
                return rc;
            HIPCHK(dout.download(out, out_bytes));
            return BPP_OK;
        });
    });
}

// The verifier's back end -- everything of a pass behind the scalar stage: k_var_digits, k_var_tables, k_var_windows,
// k_fixed_msm with its Horner stage, the folds, k_finalize(_tree) -- on MulVec scalars the caller chooses.
//   m_view: 0 = the verifier's own shape; a power of two below m = the prefix view (n, m_view) of its tables, as the
//     passes of a mixed batch use it.  N and NV below are that shape's.
//   d_points [count][NV][PW] wire records as bpp_verifier_run takes them; d_scalars [count][N][4]: the MulVec's scalars,
//     canonical (< r), in MulVec order (head, g, h, L.., R.., G.., H.., V..); d_ok, d_workspace, d_out_result [count][PW]
//     (may be null), stream: as bpp_verifier_run's.  All device buffers.
//   out_geometry (host, may be null): [Horner form as launched: 0, 1, 2, or 3 = lone; blocks per proof]
extern "C" size_t bpp_debug_verifier_mulvec_workspace_bytes(const bpp_verifier* v, size_t count, uint32_t m_view) {
    uint32_t cls = 0;
    if (!v || count > 0x7fffffffu / 64 || !debug_view_shape(v, m_view, cls)) return 0;
    size_t r = 0;
    (void)guarded([&] {
        return dispatch(v->ctx.curve, [&](auto cv) -> int {
            using V = VerifyImpl<decltype(cv)>;
            r = V::ws_layout(V::class_shape(v, cls).s, count).total;
            return 0;
        });
    });
    return r;
}
extern "C" int bpp_debug_verifier_mulvec(bpp_verifier* v, uint32_t m_view, const uint64_t* d_points, const uint64_t* d_scalars,
                                         size_t count, uint32_t* d_ok, void* d_workspace, size_t workspace_bytes,
                                         uint64_t* d_out_result, uint32_t* out_geometry, void* stream) {
    if (!v || !d_points || !d_scalars || !d_ok || !d_workspace) return fail(BPP_E_ARG, "null argument");
    if (count == 0) return BPP_OK;
    if (count > 0x7fffffffu / 64) return fail(BPP_E_ARG, "count too large for one launch");
    if (workspace_bytes == 0) return fail(BPP_E_ARG, "workspace too small");   // before the handle is read
    uint32_t cls = 0;
    if (!debug_view_shape(v, m_view, cls)) return fail(BPP_E_ARG, "m_view must be 0 or a power of two below m");
    return guarded(Count{count, "count"}, [&]() -> int {
        HIPCHK(hipSetDevice(v->ctx.device));
        return dispatch(v->ctx.curve, [&](auto cv) -> int {
            using V = VerifyImpl<decltype(cv)>;
            const VerifyShape s = V::class_shape(v, cls).s;
            if (workspace_bytes < V::ws_layout(s, count).total) return fail(BPP_E_ARG, "workspace too small");
            const size_t sc_bytes = count * (size_t)s.N * 32;
            const int rc = V::run_stage(
                v, s, d_points, count,
                [&](uint32_t* w_sc, uint32_t*, uint32_t*, hipStream_t st) -> int {
                    HIPCHK(hipMemcpyAsync(w_sc, d_scalars, sc_bytes, hipMemcpyDeviceToDevice, st));
                    return BPP_OK;
                },
                d_ok, d_workspace, workspace_bytes, nullptr, d_out_result, static_cast<hipStream_t>(stream));
            if (rc == BPP_OK && out_geometry) {
                out_geometry[0] = v->last_horner_form;
                out_geometry[1] = v->last_blocks_per_proof;
            }
            return rc;
        });
    });
}

// The many-key scan behind its decoder and its transcript -- k_recover_coeffs and k_scan_keys through
// RecoverKeysImpl::call_job, bind_class, launch_coeffs and launch_scan_keys, the functions the scan and the find call run a
// class with -- on proof scalars and challenges the caller chooses.  Host pointers, synchronous, no kernel of its own.
//   m_view: as for bpp_debug_verifier_mulvec above; k and m are that shape's.
//   scalars3 [count][3][4]: r', s', delta' ; challenges [count][3 + k][4]: y, z, e, e_1..e_k per launch position, canonical
//   status_in [count]: the decoder's word per launch position (null: zeros) ; caller [count]: the caller position of each
//     launch position, each below total (null: the identity) ; total >= count: the caller positions of the call
//   keys [n_keys][32] ; index_base, index [total] (or null): the blinding index of a caller position
//   out_coeffs [count][2k + 4][4]: [A0, c_alpha, c_delta, c_eta, c_dL.., c_dR..], canonical ; out_bad [count]
//   out_masks [n_keys][total][4], out_status [n_keys][total]: uploaded as the caller filled them, then downloaded, so a place
//     no launch position names comes back as it went in.  n_keys = 0: the coefficients alone.
extern "C" int bpp_debug_scan_keys(bpp_verifier* v, uint32_t m_view, const uint64_t* scalars3, const uint64_t* challenges,
                                   const uint32_t* status_in, const uint32_t* caller, size_t count, size_t total,
                                   const uint8_t* keys, size_t n_keys, uint64_t index_base, const uint64_t* index,
                                   uint64_t* out_coeffs, uint32_t* out_bad, uint64_t* out_masks, uint32_t* out_status) {
    if (!v || !scalars3 || !challenges || !out_coeffs || !out_bad) return fail(BPP_E_ARG, "null argument");
    if (n_keys && (!keys || !out_masks || !out_status)) return fail(BPP_E_ARG, "null argument");
    uint32_t cls = 0;
    if (!debug_view_shape(v, m_view, cls)) return fail(BPP_E_ARG, "m_view must be 0 or a power of two below m");
    if (count == 0) return BPP_OK;   // before any launch -- and before total and caller are looked at: there is nothing to place
    if (total < count) return fail(BPP_E_ARG, "total must be at least count");
    // n_keys x total (>= n_keys x count) within the bound the scan's entry puts on its pairs, without a product that can wrap
    const size_t bound = 0x7fffffffu / 64;
    if (n_keys > bound || total > bound || (n_keys && total > bound / n_keys))
        return fail(BPP_E_ARG, "n_keys x count too large for one launch");
    if (caller)
        for (size_t i = 0; i < count; i++)
            if (caller[i] >= total) return fail(BPP_E_ARG, "caller position beyond total");
    return guarded(Count{total, "total"}, [&]() -> int {
        HIPCHK(hipSetDevice(v->ctx.device));
        return dispatch(v->ctx.curve, [&](auto cv) -> int {
            using C = decltype(cv);
            using P = typename C::Fr;
            using K = RecoverKeysImpl<C>;
            typename VerifyImpl<C>::ClassView view;
            view.c = cls;
            view.ps = VerifyImpl<C>::class_shape(v, cls);
            const uint32_t k = view.ps.s.k;
            // not reachable today (make_shape: n, m <= 64, so k <= 12): kept beside check_classes of recover.hpp, which
            // says the same of the public entries
            if (k + 2 > RECOVER_GROUP) return fail(BPP_E_ARG, "mask recovery takes shapes with log2(n m) <= 14");
            const size_t ne = coeff_elems(k), pairs = n_keys * total;
            std::vector<uint32_t> rx(count * RX_WORDS, 0u);
            for (size_t i = 0; i < count; i++) rx[i * RX_WORDS + RX_CALLER] = caller ? caller[i] : (uint32_t)i;
            const std::vector<uint32_t> zeros(count, 0u);
            DevBuf dsc, dch, drx, dst, dix, dco, dbad, dom, dos, dk(true);   // dk: the keys, wiped before they are freed
            HIPCHK(dsc.upload(scalars3, count * 96));
            HIPCHK(dch.upload(challenges, count * (size_t)(3 + k) * 32));
            HIPCHK(drx.upload(rx.data(), rx.size() * 4));
            HIPCHK(dst.upload(status_in ? status_in : zeros.data(), count * 4));
            HIPCHK(dix.upload(index, total * 8));   // null: no index
            HIPCHK(dco.alloc(count * ne * K::CW * 4));
            HIPCHK(dbad.alloc(count * 4));
            view.first = 0;
            view.count = count;
            view.pts = nullptr;
            view.sc3 = dsc.u64();
            view.challenges = dch.u64();
            if (n_keys) {
                HIPCHK(dk.upload(keys, n_keys * 32));
                HIPCHK(dom.upload(out_masks, pairs * 32));
                HIPCHK(dos.upload(out_status, pairs * 4));
            }
            ScanKeysJob j = K::call_job(dk.u8(), n_keys, index_base, dix.u64(), total);
            j.out_masks = dom.u32();
            j.out_status = dos.u32();
            K::bind_class(view, drx.u32(), dst.u32(), dbad.u32(), dco.u32(), j);
            if (int rc = K::launch_coeffs(view, dco.u32(), dbad.u32(), nullptr)) return rc;
            if (n_keys)
                if (int rc = K::launch_scan_keys(j, nullptr)) return rc;
            std::vector<uint32_t> co(count * ne * K::CW);
            HIPCHK(dco.download(co.data(), co.size() * 4));
            HIPCHK(dbad.download(out_bad, count * 4));
            if (n_keys) {
                HIPCHK(dom.download(out_masks, pairs * 32));
                HIPCHK(dos.download(out_status, pairs * 4));
            }
            uint32_t* oc = reinterpret_cast<uint32_t*>(out_coeffs);
            for (size_t i = 0; i < count * ne; i++) {
                Fe<P> f;
                for (int t = 0; t < P::NL; t++) f.l[t] = co[i * K::CW + t];
                fe_to_canonical(f, oc + i * 8);
            }
            return BPP_OK;
        });
    });
}

// The batched prover's scalar stage -- k_pb_init(PB_ALL), the k whole rounds and k_pb_final through
// ProveBatchImpl::prove_batch_device's literal path (prove_layout, chunk_blinding, argument: the functions every prove entry
// runs), then the prover's own MulVec over every virtual proof -- on witnesses, blinding and challenges the caller chooses.
// Host pointers, synchronous, no kernel of its own.
//   m_view: as for bpp_debug_verifier_mulvec above; k, m and N are that shape's.  flags: BPP_PROVE_AMOUNT64 or 0.
//   values [count][m] u64 ; gammas [count][m][4] ; blinding [count][5 + 2k][4] (null: the literals), all canonical
//   challenges [count][3 + k][4]: y, z, e, e_1..e_k per proof, canonical, read at stride 3 + k (null: the shape's literals,
//     one block at stride 0).  y and every e_t must be NON-ZERO mod r: the whole kernels invert [y, e_1..e_k] with one
//     batched inversion, so a single zero among them zeroes every inverse of the proof (the transcript halves call fe_inv
//     per challenge; neither mode can meet a zero short of a zero hash).  z and e may be zero.
//   out_vps [count][2k + 3 + m][N][4]: the virtual-proof scalar arrays as the kernels leave them (pb_num_vps's numbering,
//     MulVec order, canonical; the H terms of range A are +1: k_fixed_msm negates the table entries instead)
//   out_scalars3 [count][3][4]: r', s', delta' ; out_points (may be null) [count][3 + 2k + m] wire points: the record
//     [A, wip.A, wip.B, L.., R..], then the commitments.  count: at most one chunk (prove_chunk).
extern "C" int bpp_debug_prover_scalars(bpp_verifier* v, uint32_t m_view, uint32_t flags, const uint64_t* values,
                                        const uint64_t* gammas, const uint64_t* blinding, const uint64_t* challenges, size_t count,
                                        uint64_t* out_vps, uint64_t* out_scalars3, uint64_t* out_points) {
    if (!v || !values || !gammas || !out_vps || !out_scalars3) return fail(BPP_E_ARG, "null argument");
    if (flags & ~(uint32_t)BPP_PROVE_AMOUNT64) return fail(BPP_E_ARG, "flags: BPP_PROVE_AMOUNT64 or 0");
    uint32_t cls = 0;
    if (!debug_view_shape(v, m_view, cls)) return fail(BPP_E_ARG, "m_view must be 0 or a power of two below m");
    if (count == 0) return BPP_OK;
    if (count > 2048) return fail(BPP_E_ARG, "count beyond one chunk");   // prove_chunk's cap, before any product
    return guarded(Count{count, "count"}, [&]() -> int {
        HIPCHK(hipSetDevice(v->ctx.device));
        return dispatch(v->ctx.curve, [&](auto cv) -> int {
            using C = decltype(cv);
            using PB = ProveBatchImpl<C>;
            constexpr size_t WB = (size_t)PB::WW * 4;   // bytes of a wire point
            const PassShape ps = VerifyImpl<C>::class_shape(v, cls);
            const VerifyShape& s = ps.s;
            const uint32_t k = s.k, m = s.m;
            if (count > PB::prove_chunk(s, count)) return fail(BPP_E_ARG, "count beyond one chunk");
            const typename PB::ProveLayout L = PB::prove_layout(s, count);
            const size_t vps_bytes = count * (size_t)pb_num_vps(k, m) * s.N * 32;
            const size_t rec_bytes = count * (size_t)(3 + 2 * k) * WB, V_bytes = count * (size_t)m * WB;
            DevBuf dv, dg, dbl, dch, dpts, dV, dsc, dws;
            HIPCHK(dv.upload(values, count * m * 8));
            HIPCHK(dg.upload(gammas, count * (size_t)m * 32));
            HIPCHK(dbl.upload(blinding, count * (size_t)pb_blind_elems(k) * 32));   // null: the literals
            HIPCHK(dch.upload(challenges, count * (size_t)(3 + k) * 32));          // null: the shape's literals
            HIPCHK(dpts.alloc(rec_bytes));
            HIPCHK(dV.alloc(V_bytes));
            HIPCHK(dsc.alloc(count * 96));
            HIPCHK(dws.alloc(L.total));
            ProveArgs a;   // literal mode at fixed strides, on the view's shape and the caller's challenges
            a.values = dv.u64(); a.gammas = dg.u64(); a.count = count;
            a.amount64 = (flags & BPP_PROVE_AMOUNT64) != 0; a.blinding = dbl.u64();
            a.out_points = dpts.u64(); a.out_scalars = dsc.u64(); a.out_V = dV.u64();
            a.in.ps = &ps; a.in.challenges = dch.u64();
            BPP_TRY(PB::prove_batch_device(v, a, dws.p, L.total, nullptr));
            HIPCHK(hipDeviceSynchronize());
            HIPCHK(hipMemcpy(out_vps, dws.u8() + L.vps, vps_bytes, hipMemcpyDeviceToHost));
            HIPCHK(dsc.download(out_scalars3, count * 96));
            if (out_points) {
                std::vector<uint8_t> rec(rec_bytes), V(V_bytes);
                HIPCHK(dpts.download(rec.data(), rec_bytes));
                HIPCHK(dV.download(V.data(), V_bytes));
                uint8_t* o = reinterpret_cast<uint8_t*>(out_points);
                const size_t rb = (size_t)(3 + 2 * k) * WB, vb = (size_t)m * WB;
                for (size_t p = 0; p < count; p++) {
                    std::memcpy(o + p * (rb + vb), rec.data() + p * rb, rb);
                    std::memcpy(o + p * (rb + vb) + rb, V.data() + p * vb, vb);
                }
            }
            return BPP_OK;
        });
    });
}

// The verifier's window tables read back: entries first .. first + count - 1 of one generator, T[j][d] = d 2^(off_j) F at
// entry went[j] + d - 1 (fixed_glv.hpp).  Host pointers, synchronous, no kernel of its own.
//   generator: TABLE numbering, [0, NF) of the verifier's own shape (g, h, G_0.., H_0..); first + count <= per_f
//   out_raw [count][2N] (may be null): the device words of the entries exactly as stored, one device-to-host copy
//   out_wire [count][PW] (may be null): the same entries through k_points_to_wire
//   out_layout (may be null): [W, top, per_f, glv, hgap, slabs, runs_per_generator], then wc[0..W), then went[0..W), as the
//     verifier's shape carries them; slabs = the k_tbl_fill launches create made, runs_per_generator = the runs of TBL_RUN
//     entries it gave each generator.  Written whatever count is.
extern "C" int bpp_debug_verifier_table(bpp_verifier* v, uint32_t generator, uint32_t first, uint32_t count, uint32_t* out_raw,
                                        uint64_t* out_wire, uint32_t* out_layout) {
    if (!v) return fail(BPP_E_ARG, "null argument");
    const VerifyShape& s = v->s;
    if (generator >= s.NF) return fail(BPP_E_ARG, "generator beyond the table");
    if (first > s.per_f || count > s.per_f - first) return fail(BPP_E_ARG, "entries beyond the generator's table");
    return guarded([&]() -> int {
        if (out_layout) {
            const uint32_t head[7] = {s.W, s.top, s.per_f, s.glv, s.hgap, v->table_slabs, v->table_runs_per_generator};
            std::memcpy(out_layout, head, sizeof head);
            for (uint32_t j = 0; j < s.W; j++) {
                out_layout[7 + j] = s.wc[j];
                out_layout[7 + s.W + j] = s.went[j];
            }
        }
        if (count == 0 || (!out_raw && !out_wire)) return BPP_OK;
        HIPCHK(hipSetDevice(v->ctx.device));
        return dispatch(v->ctx.curve, [&](auto cv) -> int {
            return VerifyImpl<decltype(cv)>::table_slice(v, generator, first, count, out_raw, out_wire);
        });
    });
}
