// wip_seam.hpp -- WeightedInnerProductProof::{prove, verify} as a batched seam of its own (bpp_wip_prove_batch_device,
// bpp_wip_verify_batch_device): the kernels that the range statement's passes do not have.
//
// Reference: src/weighted_inner_product_proof.rs:36-227 (prove), :238-328 (verify), :330-382 (verification_scalars).
//
// The relation:  P = sum a_i G_i + sum b_i H_i + (sum a_i b_i y^(i+1)) g + gamma h  over the engine's key, len = n m.
// power_of_y_vec is [y, y^2, .., y^len]: the reference's verify reads only its first entry and rebuilds the rest
// (wip.rs:252, :276) and both of its callers hand the prover exactly this vector, so the seam takes the scalar y.
// prove's `commitment` argument is dead in the reference (wip.rs:57, :137-142) and is not taken.
//
// Prover: k_wip_init stands where k_pb_init stands in the range prover (prover_batch.hpp) -- the caller's a, b, y, gamma
// instead of the bits of v -- and the rounds, the final step, the MulVecs over the window tables and the collection of the
// wire points are the range prover's own kernels, run over the 2k + 2 virtual proofs 1 .. 2k+2 (there is no range A and
// there are no commitments).  Records go through the px index (PX_REC) to a stride of 3 + 2k + nv wire points; point 0
// (A') and the last nv (V) belong to the caller and are not touched.
//
// Verifier: k_wvs_prepare / k_wvs_expand stand where k_vs_prepare / k_vs_expand stand, with the caller's statement
// [Gc (len), Hc (len), gc, Vc (nv)] -- the four *_exp_of_commitment arguments of wip.rs:238-247 -- in place of the range
// statement's y, z, n, m:
//   scalars [1, e, e^2, g_exp, h_exp, e_j^2 e^2 (k), e_j^-2 e^2 (k), G_exp (len), H_exp (len), V_exp (nv)]
//   points  [B, A, A', g, h, L.., R.., G_vec, H_vec, V..]                                          (wip.rs:298-316)
//   G_exp[i] = -s[i] y^-(i+1) r' e y + Gc[i] e^2      H_exp[i] = -s[len-1-i] s' e + Hc[i] e^2
//   g_exp = -r' y s' + gc e^2      h_exp = -delta'      V_exp[j] = Vc[j] e^2
// with s[i] = prod_j e_j^-1 * prod_{bit b of i set} e_{k-1-b}^2 (wip.rs:372-380).
//
// Transcript: the argument continues a transcript the caller owns -- 32 bytes of running state per proof, after the
// caller absorbed its statement and drew y -- with dsep "wipp v1\0", n = len, then per round L_t, R_t -> e_t, then
// wA, wB -> e (transcript.hpp; the same steps as the range argument's tail).
#pragma once
#include "prover_batch.hpp"

namespace bpp {

// the literal challenges of the reference (wip.rs:131 / :353, :211 / :369)
struct WipLiterals {
    uint32_t e_round, e_final;
};

// ---- prover ------------------------------------------------------------------------------------------------------

// px entries of a chunk (prover_batch.hpp PX_*): proof base + p writes its record at wire point (base + p) * rec_stride
// and its scalar triple / blinding index at caller position base + p
static __global__ void __launch_bounds__(256) k_wip_px(uint32_t* __restrict__ px, size_t base, uint32_t rec_stride, size_t cnt) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= cnt) return;
    uint32_t* e = px + p * PX_WORDS;
    for (int i = 0; i < PX_WORDS; i++) e[i] = 0;
    e[PX_REC] = (uint32_t)((base + p) * rec_stride);
    e[PX_CALLER] = (uint32_t)(base + p);
}

// One block (256 threads) per proof; s: the seam's prover shape (m = 0, 2k + 3 virtual-proof slots, slot 0 unused).
// a_in, b_in: [count][mn][8] canonical ; y_in, gamma_in: [count][8].  fs = 0: the literal challenges and their inverses
// are filled in here (one batched inversion with y); fs = 1: only y^-1 (e_t, e_t^-1, e arrive from k_pb_fs_round / _final).
template <class C>
__global__ void __launch_bounds__(256) k_wip_init(VerifyShape s, WipLiterals lit, uint32_t fs,
                                                  const uint32_t* __restrict__ a_in, const uint32_t* __restrict__ b_in,
                                                  const uint32_t* __restrict__ y_in, const uint32_t* __restrict__ gamma_in,
                                                  uint32_t* __restrict__ st_a, uint32_t* __restrict__ st_b,
                                                  uint32_t* __restrict__ st_cG, uint32_t* __restrict__ st_cH,
                                                  uint32_t* __restrict__ st_pwy, uint32_t* __restrict__ st_consts,
                                                  uint32_t* __restrict__ vps) {
    using P = typename C::Fr;
    using F = Fe<P>;
    __shared__ F sh_ypw[VS_MAXK + 2];
    const uint32_t tid = threadIdx.x;
    const size_t p = blockIdx.x;
    const uint32_t k = s.k, mn = s.mn;
    uint32_t* consts = st_consts + p * (size_t)pb_consts_elems(k) * 8;
    const uint32_t nvp = pb_num_vps(k, s.m);
    // zero the scalar arrays of virtual proofs 1 .. nvp-1 (slot 0, the range prover's A, is never read)
    {
        uint4* q = reinterpret_cast<uint4*>(vps + (p * nvp + 1) * (size_t)s.N * 8);
        const size_t n16 = (size_t)(nvp - 1) * s.N * 2;
        for (size_t t = tid; t < n16; t += blockDim.x) q[t] = make_uint4(0, 0, 0, 0);
    }
    if (tid == 0) {
        uint32_t w[8];
        ld_words<8>(y_in + p * 8, w);
        const F y = fe_from_canonical<P>(w);
        ld_words<8>(gamma_in + p * 8, w);
        pb_st<P>(consts + 1 * 8, fe_from_canonical<P>(w));   // alpha_w = gamma                      (wip.rs:69)
        pb_st<P>(consts + 2 * 8, y);
        pb_st<P>(consts + 3 * 8, F::zero());                 // the range statement's z: not part of the seam
        if (fs) {
            pb_st<P>(consts + 0, fe_inv(y));
        } else {
            const F e = fe_from_u32<P>(lit.e_round);
            pb_st<P>(consts + 4 * 8, fe_from_u32<P>(lit.e_final));
            F acc = y.is_zero() ? F::one() : y;   // prefix products kept in the e^-1 slots
            for (uint32_t t = 0; t < k; t++) {
                pb_st<P>(consts + (5 + t) * 8, e);
                pb_st<P>(consts + (5 + k + t) * 8, acc);
                acc = fe_mul(acc, e);
            }
            F inv = fe_inv(acc);
            for (uint32_t t = k; t-- > 0;) {
                const F pre = pb_ld<P>(consts + (5 + k + t) * 8);
                pb_st<P>(consts + (5 + k + t) * 8, fe_mul(inv, pre));   // e_t^-1
                inv = fe_mul(inv, e);
            }
            pb_st<P>(consts + 0, y.is_zero() ? F::zero() : inv);        // y^-1
        }
        F yy = y;
        for (uint32_t bnum = 0; bnum <= k + 1; bnum++) {
            sh_ypw[bnum] = yy;
            yy = fe_sqr(yy);
        }
    }
    __syncthreads();
    const F one = F::one();
    for (uint32_t i = tid; i < mn; i += blockDim.x) {
        F yp = one;   // y^(i+1)
        const uint32_t e1 = i + 1;
        for (uint32_t bnum = 0; bnum <= k; bnum++)
            if ((e1 >> bnum) & 1u) yp = fe_mul(yp, sh_ypw[bnum]);
        uint32_t w[8];
        ld_words<8>(a_in + (p * mn + i) * 8, w);
        pb_st<P>(st_a + (p * mn + i) * 8, fe_from_canonical<P>(w));
        ld_words<8>(b_in + (p * mn + i) * 8, w);
        pb_st<P>(st_b + (p * mn + i) * 8, fe_from_canonical<P>(w));
        pb_st<P>(st_pwy + (p * mn + i) * 8, yp);
        pb_st<P>(st_cG + (p * mn + i) * 8, one);
        pb_st<P>(st_cH + (p * mn + i) * 8, one);
    }
}

// the 32 state bytes the caller hands over -> the eight state words of transcript.hpp (big-endian words of the digest)
__device__ __forceinline__ void wip_load_state(const uint8_t* __restrict__ bytes, Transcript& t) {
    for (int i = 0; i < 8; i++)
        t.st[i] = ((uint32_t)bytes[4 * i] << 24) | ((uint32_t)bytes[4 * i + 1] << 16) | ((uint32_t)bytes[4 * i + 2] << 8) |
                  (uint32_t)bytes[4 * i + 3];
}
__device__ __forceinline__ void wip_transcript_start(Transcript& t, uint32_t mn) {
    const uint32_t dsep[2] = {tr_tag('w', 'i', 'p', 'p'), tr_tag(' ', 'v', '1', 0)};
    tr_append_words(t, tr_tag('d', 's', 'e', 'p'), dsep, 2);
    tr_append_u64(t, tr_tag('n'), mn);
}

// one lane per proof: the caller's state plus the argument's separator (what k_pb_fs_yz leaves for the range prover)
template <class C>
__global__ void __launch_bounds__(64) k_wip_fs_start(VerifyShape s, const uint8_t* __restrict__ states,
                                                     uint32_t* __restrict__ tr_st, size_t count) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= count) return;
    Transcript t;
    wip_load_state(states + p * 32, t);
    wip_transcript_start(t, s.mn);
    for (int i = 0; i < 8; i++) tr_st[p * 8 + i] = t.st[i];
}

// one wave per proof: [e, e_1..e_k] out of the prover's block [y, z, e, e_1..e_k] (ch == null: the literals)
template <class C>
__global__ void __launch_bounds__(64) k_wip_challenges_out(uint32_t k, WipLiterals lit, const uint32_t* __restrict__ ch,
                                                           uint32_t* __restrict__ out) {
    const size_t p = blockIdx.x;
    const uint32_t nw = (1 + k) * 8;
    for (uint32_t w = threadIdx.x; w < nw; w += 64) {
        uint32_t x;
        if (ch) x = ch[p * (size_t)(3 + k) * 8 + 16 + w];
        else x = (w & 7u) ? 0u : (w == 0 ? lit.e_final : lit.e_round);
        out[p * nw + w] = x;
    }
}

// ---- verifier ----------------------------------------------------------------------------------------------------

// one lane per proof: seed state and record [A', wip.A, wip.B, L.., R.., V..] -> [e, e_1..e_k]
template <class C>
__global__ void __launch_bounds__(64) k_wip_transcript_challenges(VerifyShape s, const uint8_t* __restrict__ states,
                                                                  const uint32_t* __restrict__ records,
                                                                  uint32_t* __restrict__ challenges, size_t count) {
    using P = typename C::Fr;
    constexpr uint32_t WW = 2 * C::Fp::N + 2;
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= count) return;
    const uint32_t k = s.k;
    const uint32_t* rec = records + b * (size_t)s.NV * WW;
    uint32_t* out = challenges + b * (size_t)(1 + k) * 8;
    Transcript t;
    wip_load_state(states + b * 32, t);
    wip_transcript_start(t, s.mn);
    uint32_t w[8];
    for (uint32_t r = 0; r < k; r++) {
        tr_append_point<C>(t, tr_tag('L'), rec + (size_t)(3 + r) * WW);
        tr_append_point<C>(t, tr_tag('R'), rec + (size_t)(3 + k + r) * WW);
        fe_to_canonical(tr_challenge<P>(t, tr_tag('e')), w);
        for (int i = 0; i < 8; i++) out[(size_t)(1 + r) * 8 + i] = w[i];
    }
    tr_append_point<C>(t, tr_tag('w', 'A'), rec + (size_t)1 * WW);
    tr_append_point<C>(t, tr_tag('w', 'B'), rec + (size_t)2 * WW);
    fe_to_canonical(tr_challenge<P>(t, tr_tag('e')), w);
    for (int i = 0; i < 8; i++) out[i] = w[i];
}

// per-proof block of `prep` (k_wvs_prepare -> k_wvs_expand, through LDS)
template <class F>
struct WvsShared {
    F* chsq;    // [k]    e_j^2
    F* yipw;    // [k+1]  y^-(2^b)
    F* sy_lo;   // [CH]   prod_{low bits of l set} e^2 * y^-l
    F* sc_lo;   // [CH]   prod_{low bits of l unset} e^2
    F* tmp;     // [k+1]  prefix products of the batched inversion, then the e_j^-1
    F* c;       // [4]    kGa, kHa, e^2
    __host__ __device__ static uint32_t elems(uint32_t k, uint32_t CH) { return k + (k + 1) + 2 * CH + (k + 1) + 4; }
    __device__ WvsShared(F* base, uint32_t k, uint32_t CH) {
        chsq = base;
        yipw = chsq + k;
        sy_lo = yipw + k + 1;
        sc_lo = sy_lo + CH;
        tmp = sc_lo + CH;
        c = tmp + k + 1;
    }
    __device__ F& kGa() { return c[0]; }
    __device__ F& kHa() { return c[1]; }
    __device__ F& esq() { return c[2]; }
};
__host__ __device__ inline uint32_t wvs_ch(const VerifyShape& s) { return s.mn >= 64 ? s.mn / 64 : 1; }
template <class C>
inline size_t wvs_prep_bytes(const VerifyShape& s) {
    using F = Fe<typename C::Fr>;
    return (size_t)WvsShared<F>::elems(s.k, wvs_ch(s)) * sizeof(F);
}
template <class C>
inline size_t wvs_lds_bytes(const VerifyShape& s) {
    return (size_t)VS_PB * wvs_prep_bytes<C>(s);
}
// scalars of one proof's statement block [Gc (mn), Hc (mn), gc, Vc (nv)]
__host__ __device__ inline uint32_t wip_statement_elems(const VerifyShape& s) { return 2 * s.mn + 1 + s.m; }

// ONE LANE PER PROOF: what is serial per proof.  s: the seam's pass shape (m = nv).  proof_scalars: [r', s', delta'] ;
// y_in: [count][8] ; statement: [count][2 mn + 1 + nv][8] ; challenges: [e, e_1..e_k] per proof (null: the literals).
// y = 0 (mod r) has no inverse: the proof is marked invalid (bad[b], the flag the invalid wire points raise).
template <class C>
__global__ void __launch_bounds__(64) k_wvs_prepare(VerifyShape s, WipLiterals lit, const uint32_t* __restrict__ proof_scalars,
                                                    const uint32_t* __restrict__ y_in, const uint32_t* __restrict__ statement,
                                                    const uint32_t* __restrict__ challenges, uint32_t* __restrict__ prep,
                                                    uint32_t* __restrict__ out, uint32_t* __restrict__ bad, size_t count) {
    using P = typename C::Fr;
    using F = Fe<P>;
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= count) return;
    const uint32_t k = s.k, mn = s.mn, nv = s.m;
    const uint32_t CH = wvs_ch(s);
    WvsShared<F> sh(reinterpret_cast<F*>(prep) + b * WvsShared<F>::elems(k, CH), k, CH);
    const uint32_t* ch = challenges ? challenges + b * (size_t)(1 + k) * 8 : nullptr;
    const uint32_t* stm = statement + b * (size_t)wip_statement_elems(s) * 8;
    uint32_t* o = out + b * (size_t)s.N * 8;
    uint32_t w[8];
    auto chal = [&](uint32_t j) -> F {   // 0: e, 1 + t: e_t
        if (!ch) return fe_from_u32<P>(j ? lit.e_round : lit.e_final);
        uint32_t cw[8];
        ld_words<8>(ch + (size_t)j * 8, cw);
        return fe_from_canonical<P>(cw);
    };
    ld_words<8>(y_in + b * 8, w);
    const F y = fe_from_canonical<P>(w);
    if (y.is_zero()) bad[b] = 1u;
    // ---- inverses of [y, e_1..e_k]: one safegcd call; zero entries are skipped (their "inverse" stays 0)
    F yinv, allinv = F::one();
    {
        F acc = F::one();
        for (uint32_t j = 0; j <= k; j++) {
            const F x = j ? chal(j) : y;
            if (!x.is_zero()) acc = fe_mul(acc, x);
            sh.tmp[j] = acc;
        }
        F inv = fe_inv(acc);
        yinv = F::zero();
        for (uint32_t j = k + 1; j-- > 0;) {
            const F x = j ? chal(j) : y;
            F xi = F::zero();
            if (!x.is_zero()) {
                xi = j ? fe_mul(inv, sh.tmp[j - 1]) : inv;
                inv = fe_mul(inv, x);
            }
            if (j == 0) yinv = xi;
            else {
                sh.chsq[j - 1] = fe_sqr(x);
                sh.tmp[j] = xi;
                allinv = fe_mul(allinv, xi);
            }
        }
    }
    const F e = chal(0);
    const F esq = fe_sqr(e);
    ld_words<8>(proof_scalars + b * 24, w);
    const F rp = fe_from_canonical<P>(w);
    ld_words<8>(proof_scalars + b * 24 + 8, w);
    const F sp = fe_from_canonical<P>(w);
    ld_words<8>(proof_scalars + b * 24 + 16, w);
    const F dp = fe_from_canonical<P>(w);
    sh.kGa() = fe_mul(fe_mul(fe_mul(rp, e), y), allinv);   // r' e y allinv
    sh.kHa() = fe_mul(fe_mul(sp, e), allinv);              // s' e allinv
    sh.esq() = esq;
    // head scalars                                                                       (wip.rs:298-302)
    ld_words<8>(stm + (size_t)2 * mn * 8, w);
    const F gc = fe_from_canonical<P>(w);
    fe_to_canonical(F::one(), w);
    st_words<8>(o + 0, w);
    fe_to_canonical(e, w);
    st_words<8>(o + 8, w);
    fe_to_canonical(esq, w);
    st_words<8>(o + 16, w);
    fe_to_canonical(fe_sub(fe_mul(gc, esq), fe_mul(fe_mul(rp, y), sp)), w);   // g_exp           (:286-289)
    st_words<8>(o + 24, w);
    fe_to_canonical(fe_neg(dp), w);                                           // h_exp           (:291)
    st_words<8>(o + 32, w);
    for (uint32_t j = 0; j < k; j++) {                                        // Ls_exp, Rs_exp  (:264-273)
        fe_to_canonical(fe_mul(sh.chsq[j], esq), w);
        st_words<8>(o + (size_t)(5 + j) * 8, w);
        fe_to_canonical(fe_mul(fe_sqr(sh.tmp[j + 1]), esq), w);
        st_words<8>(o + (size_t)(5 + k + j) * 8, w);
    }
    for (uint32_t j = 0; j < nv; j++) {                                       // V_exp           (:293-296)
        ld_words<8>(stm + (size_t)(2 * mn + 1 + j) * 8, w);
        fe_to_canonical(fe_mul(fe_from_canonical<P>(w), esq), w);
        st_words<8>(o + (size_t)(5 + 2 * k + 2 * mn + j) * 8, w);
    }
    F yi = yinv;
    for (uint32_t bnum = 0; bnum <= k; bnum++) {
        sh.yipw[bnum] = yi;
        yi = fe_sqr(yi);
    }
}

// VS_PB proofs per block, 64 lanes per proof, mn/64 consecutive indices each (k_vs_expand's geometry and product tables):
//   G_exp[i] = Gc[i] e^2 - [kGa prod_{hi bits set} e^2 y^-(i0+1)] * sy_lo[l]
//   H_exp[i] = Hc[i] e^2 - [kHa prod_{hi bits unset} e^2] * sc_lo[l]                                   i = i0 + l
template <class C>
__global__ void __launch_bounds__(VS_BLOCK) k_wvs_expand(VerifyShape s, const uint32_t* __restrict__ prep,
                                                         const uint32_t* __restrict__ statement, uint32_t* __restrict__ out,
                                                         size_t count) {
    using P = typename C::Fr;
    using F = Fe<P>;
    extern __shared__ __align__(16) uint32_t lds_raw[];
    const uint32_t tid = threadIdx.x;
    const uint32_t k = s.k, mn = s.mn;
    const uint32_t CH = wvs_ch(s);
    uint32_t cb = 0;
    while ((1u << cb) < CH) cb++;
    const uint32_t per_proof = WvsShared<F>::elems(k, CH);
    {
        const size_t first = (size_t)blockIdx.x * VS_PB;
        const size_t nproofs = count - first < VS_PB ? count - first : VS_PB;
        const size_t words = nproofs * per_proof * (sizeof(F) / 4);
        const uint32_t* src = prep + first * per_proof * (sizeof(F) / 4);
        for (size_t t = tid; t < words; t += blockDim.x) lds_raw[t] = src[t];
    }
    __syncthreads();
    const uint32_t q = tid / 64, lane = tid % 64;
    const size_t b = (size_t)blockIdx.x * VS_PB + q;
    const bool active = b < count;
    WvsShared<F> sh(reinterpret_cast<F*>(lds_raw) + (size_t)q * per_proof, k, CH);
    if (active && lane < CH) {
        F slo = F::one(), sclo = F::one(), yl = F::one();
        for (uint32_t bnum = 0; bnum < cb; bnum++) {
            const F u = sh.chsq[k - 1 - bnum];
            if ((lane >> bnum) & 1u) {
                slo = fe_mul(slo, u);
                yl = fe_mul(yl, sh.yipw[bnum]);
            } else {
                sclo = fe_mul(sclo, u);
            }
        }
        sh.sy_lo[lane] = fe_mul(slo, yl);
        sh.sc_lo[lane] = sclo;
    }
    __syncthreads();
    if (!active) return;
    const uint32_t i0 = lane * CH;
    if (i0 >= mn) return;
    uint32_t* o = out + b * (size_t)s.N * 8;
    const uint32_t* stm = statement + b * (size_t)wip_statement_elems(s) * 8;
    F a_hi = sh.kGa(), c_hi = sh.kHa();
    for (uint32_t bnum = cb; bnum < k; bnum++) {
        const F u = sh.chsq[k - 1 - bnum];
        if ((i0 >> bnum) & 1u) a_hi = fe_mul(a_hi, u);
        else c_hi = fe_mul(c_hi, u);
    }
    {
        const uint32_t e1 = i0 + 1;   // y^-(i0+1)
        for (uint32_t bnum = 0; bnum <= k; bnum++)
            if ((e1 >> bnum) & 1u) a_hi = fe_mul(a_hi, sh.yipw[bnum]);
    }
    const F esq = sh.esq();
    for (uint32_t l = 0; l < CH; l++) {
        const uint32_t i = i0 + l;
        uint32_t wv[8];
        ld_words<8>(stm + (size_t)i * 8, wv);
        const F ge = fe_sub(fe_mul(fe_from_canonical<P>(wv), esq), fe_mul(a_hi, sh.sy_lo[l]));
        ld_words<8>(stm + (size_t)(mn + i) * 8, wv);
        const F he = fe_sub(fe_mul(fe_from_canonical<P>(wv), esq), fe_mul(c_hi, sh.sc_lo[l]));
        fe_to_canonical(ge, wv);
        st_words<8>(o + (size_t)(5 + 2 * k + i) * 8, wv);
        fe_to_canonical(he, wv);
        st_words<8>(o + (size_t)(5 + 2 * k + mn + i) * 8, wv);
    }
}

}  // namespace bpp
