// host_util.hpp -- host-side helpers shared by capi.hip and the impl_*.hpp units (device buffers: staging.hpp, error
// state, curve dispatch, scalar canonicalisation, the MulVec launcher).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bpp_amd.h"
#include "abi_guard.hpp"
#include "kernels.hpp"

struct bpp_ctx {
    int curve;
    int device;
    // per-stage timing of bpp_msm_device (bpp_msm_set_profiling): MSM_SLOTS passes x (stages + 1) events
    bool msm_profiling = false;
    size_t msm_passes = 0;
    std::vector<hipEvent_t> msm_events;
    uint32_t msm_shape[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // of the last bpp_msm_device call: n, items, W, q, nwide, nbuckets, L, c
    // the small-table verifiers bpp_range_verify keeps per public key (literal.hpp, struct VerifyCache); owned by the
    // context that bpp_init returned -- the copies inside verifiers never touch it
    void* verify_cache = nullptr;
    bool verify_cache_off = false;
};   // (the events are destroyed by bpp_destroy: verifiers keep a COPY of their context)
constexpr size_t BPP_MSM_SLOTS = 16;

// Entry points of the per-curve implementation structs (impl_*.hpp, codec.hpp).  They are defined in class, hence
// implicitly inline, and `extern template` does not stop the compiler from instantiating an inline function in order
// to inline it: without this attribute capi.hip compiled every kernel of every curve a second time (8 minutes, 12 MB).
#define BPP_NOINL __attribute__((noinline))

#include "staging.hpp"   // HIPCHK, DevBuf: the staging vocabulary of the host forms

namespace bpp {

template <class F>
inline int dispatch(int curve, F&& f) {
    switch (curve) {
        case BPP_BLS12_381_G1: return f(Bls12381{});
        case BPP_SECP256K1: return f(Secp256k1{});
        case BPP_ED25519: return f(Ed25519{});
        default: return fail(BPP_E_ARG, "unknown curve id");
    }
}

inline unsigned cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// Lays a workspace out buffer by buffer: take(bytes) returns the next buffer's offset and reserves `bytes` rounded up to
// 256; `total` is the size of everything taken so far.
struct WsCarver {
    size_t total = 0;
    size_t take(size_t bytes) {
        const size_t o = total;
        total += (bytes + 255) & ~(size_t)255;
        return o;
    }
};

// a 32-byte key (WeightKey, BlindKey) as 8 little-endian words; null: zeros
inline void load_key_words(const uint8_t* key, uint32_t w[8]) {
    for (int i = 0; i < 8; i++)
        w[i] = key ? (uint32_t)key[4 * i] | ((uint32_t)key[4 * i + 1] << 8) | ((uint32_t)key[4 * i + 2] << 16) |
                         ((uint32_t)key[4 * i + 3] << 24)
                   : 0u;
}

// canonical (< group order) 32-byte little-endian scalar?
template <class C>
inline bool scalar_is_canonical(const uint8_t* b) {
    uint32_t w[8];
    load_key_words(b, w);
    return words_lt_mod<typename C::Fr>(w);
}

inline uint32_t log2_exact(size_t x) {
    uint32_t k = 0;
    while (((size_t)1 << k) < x) k++;
    return k;
}

// scalar (4 x u64 = 8 words) reduced mod r on the host: PrimeFieldElem values are always < r.  A 256-bit value holds up
// to floor(2^256 / r) multiples of r: 1 on secp256k1, 2 on BLS12-381, 15 on edwards25519 (r ~ 2^252) -- hence 16
// rounds, as k_pip_points does on the device
template <class C>
void reduce_scalar_words(uint32_t* w) {
    using P = typename C::Fr;
    for (int iter = 0; iter < 16; iter++) {
        if (words_lt_mod<P>(w)) return;
        uint64_t borrow = 0;
        for (int i = 0; i < 8; i++) {
            uint64_t t = (uint64_t)w[i] - P::MODW[i] - borrow;
            w[i] = (uint32_t)t;
            borrow = (t >> 32) & 1u;
        }
    }
}

// PrimeFieldElem::new(i32) as canonical words (prime_field_elem.rs:191-195)
template <class C>
void scalar_from_i32(int32_t n, uint32_t* w) {
    using P = typename C::Fr;
    for (int i = 0; i < 8; i++) w[i] = 0;
    if (n >= 0) {
        w[0] = (uint32_t)n;
        return;
    }
    uint64_t mag = (uint64_t)(-(int64_t)n);
    uint64_t borrow = 0;
    for (int i = 0; i < 8; i++) {
        uint64_t sub = (i == 0) ? (mag & 0xffffffffu) : (i == 1 ? (mag >> 32) : 0);
        uint64_t t = (uint64_t)P::MODW[i] - sub - borrow;
        w[i] = (uint32_t)t;
        borrow = (t >> 32) & 1u;
    }
}

template <class C>
constexpr int wire_words() {
    return 2 * C::Fp::N + 2;
}

// Upload wire points, convert to affm on the device.  Returns BPP_E_POINT when any is invalid.
template <class C>
int upload_points(const uint64_t* wire, size_t n, DevBuf& affm, hipStream_t st) {
    constexpr int N = C::Fp::N;
    DevBuf dw, bad;
    HIPCHK(dw.alloc(n * wire_words<C>() * 4));
    HIPCHK(bad.alloc(4));
    HIPCHK(affm.alloc(n * 2 * N * 4));
    HIPCHK(zero_words_async(bad.p, 4, st));
    if (n) {
        HIPCHK(hipMemcpyAsync(dw.p, wire, n * wire_words<C>() * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_points_from_wire<C>, dim3(cdiv(n, 128)), dim3(128), 0, st, dw.u32(), affm.u32(),
                           bad.u32(), n, 0u);
        HIPCHK(hipGetLastError());
    }
    uint32_t hbad = 0;
    HIPCHK(hipMemcpyAsync(&hbad, bad.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (hbad) return fail(BPP_E_POINT, "point not on curve / coordinate out of range");
    return BPP_OK;
}

template <class C>
int upload_scalars(const uint64_t* sc, size_t n, DevBuf& d, hipStream_t st) {
    std::vector<uint32_t> h(n * 8 + 8);
    if (n) std::memcpy(h.data(), sc, n * 32);
    for (size_t i = 0; i < n; i++) reduce_scalar_words<C>(h.data() + i * 8);
    HIPCHK(d.alloc(n * 32));
    if (n) HIPCHK(hipMemcpyAsync(d.p, h.data(), n * 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return BPP_OK;
}

template <class C>
inline void store_generator(uint32_t* affm_words) {
    Aff<C> g = aff_generator<C>();
    aff_store(g, affm_words);
}

inline bool is_pow2(size_t x) { return x && !(x & (x - 1)); }

// fr_modw: the scalar-field modulus as 8 little-endian 32-bit words, fr_bits its bit length.
// glv_half_max (4 words, or null): the table serves the two halves of the curve's endomorphism split, each at most this
// large -- the mixed-width layout of fixed_glv.hpp instead of the uniform one (make_verify_shape below).
inline int make_shape(size_t n, size_t m, int c, const uint32_t* fr_modw, int fr_bits, VerifyShape& s,
                      const uint32_t* glv_half_max = nullptr) {
    const size_t mn = n * m;
    if (n == 0 || m == 0 || !is_pow2(mn)) return fail(BPP_E_ARG, "n*m must be a power of two");
    if (n > VS_MAXN || m > VS_MAXM) return fail(BPP_E_ARG, "n or m exceeds the supported maximum (64)");
    uint32_t k = 0;
    while (((size_t)1 << k) < mn) k++;
    if (k > VS_MAXK) return fail(BPP_E_ARG, "n*m too large");
    if (c < 2 || c > 20) return fail(BPP_E_ARG, "window_bits must be in [2, 20]");
    static_assert(VS_MAXW == GLV_MAXW, "VerifyShape carries a WinLayout's windows");
    WinLayout L;
    if (glv_half_max) {
        if (!glv_layout(c, fr_bits, glv_half_max, L)) return fail(BPP_E_ARG, "window_bits too small or too large for this scalar field");
    } else if (const char* why = win_layout_uniform(c, fr_modw, fr_bits, L)) {
        return fail(BPP_E_ARG, why);
    }
    s.n = (uint32_t)n;
    s.m = (uint32_t)m;
    s.mn = (uint32_t)mn;
    s.k = k;
    s.N = (uint32_t)(2 * mn + 2 * k + m + 5);
    s.NF = (uint32_t)(2 * mn + 2);
    s.NV = (uint32_t)(3 + 2 * k + m);
    s.c = (uint32_t)c;
    s.W = L.W;
    s.top = L.top;
    s.per_f = L.per_f;
    for (int t = 0; t < WIN_FULL_WORDS; t++) s.bias[t] = L.bias[t];
    s.hgap = 0;
    s.glv = glv_half_max ? 1u : 0u;
    for (int j = 0; j < VS_MAXW; j++) {
        s.wc[j] = L.wc[j];
        s.went[j] = L.went[j];
    }
    s.head_wip = m == 1 ? 1u : 0u;
    return BPP_OK;
}

// the shape of a verifier on curve C
template <class C>
inline int make_verify_shape(size_t n, size_t m, int c, VerifyShape& s) {
    if constexpr (fixed_glv<C>()) {
        uint32_t hmax[4];
        glv_half_max<C>(hmax);
        return make_shape(n, m, c, C::Fr::MODW, C::Fr::BITS, s, hmax);
    } else {
        return make_shape(n, m, c, C::Fr::MODW, C::Fr::BITS, s);
    }
}

// the two verifier-scalars kernels (kernels.hpp): d_prep holds count * vs_prep_bytes<C>(s) bytes
template <class C>
inline int launch_verify_scalars(const VerifyShape& s, const uint32_t* d_proof_scalars, const uint32_t* d_challenges,
                                 uint32_t ch_stride, uint32_t* d_out, size_t count, uint32_t* d_prep, hipStream_t st) {
    // above the default dynamic-LDS limit: opt in (160 KB per CU on gfx950) to the largest shape seen so far -- the
    // passes of a mixed batch (bpp_verifier_run_mixed) run the smaller shapes first.  The record is kept per device (the
    // attribute belongs to the kernel's code object on the current device) and under a lock: a verifier serves several
    // host threads, and a pool (pool.hpp) runs one thread per device.
    if (vs_lds_bytes<C>(s) > 64 * 1024) {
        constexpr int MAX_DEV = 64;
        static std::mutex mu;
        static size_t lds_opted_in[MAX_DEV] = {};   // 0: the default limit
        int dev = -1;
        HIPCHK(hipGetDevice(&dev));
        const std::lock_guard<std::mutex> lock(mu);
        const bool known = dev >= 0 && dev < MAX_DEV;   // an ordinal beyond the record opts in every time
        if (!known || vs_lds_bytes<C>(s) > lds_opted_in[dev]) {
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vs_expand<C>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)vs_lds_bytes<C>(s)));
            if (known) lds_opted_in[dev] = vs_lds_bytes<C>(s);
        }
    }
    hipLaunchKernelGGL(k_vs_prepare<C>, dim3(cdiv(count, 64)), dim3(64), 0, st, s, d_proof_scalars, d_challenges, ch_stride,
                       d_prep, d_out, count);
    hipLaunchKernelGGL(k_vs_expand<C>, dim3(cdiv(count, VS_PB)), dim3(VS_BLOCK), vs_lds_bytes<C>(s), st, s, d_prep, d_out,
                       count);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

// default challenges = the reference's hard-coded "transcript" (SURVEY.md 3.4):
// [y, z, e, e_1..e_k] = m == 1 ? [7, 7, 99, 7..] : [12, 23, 99, 7..]
inline void default_challenges(const VerifyShape& s, std::vector<uint32_t>& w) {
    w.assign((size_t)(3 + s.k) * 8, 0);
    w[0] = s.m == 1 ? 7 : 12;   // range/mod.rs:198 / :417
    w[8] = s.m == 1 ? 7 : 23;   // range/mod.rs:199 / :418
    w[16] = 99;                 // wip.rs:369
    for (uint32_t j = 0; j < s.k; j++) w[(size_t)(3 + j) * 8] = 7;  // wip.rs:353
}

}  // namespace bpp

