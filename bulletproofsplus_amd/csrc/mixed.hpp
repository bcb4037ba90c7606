// mixed.hpp -- batches of mixed aggregation sizes (bpp_verifier_run_mixed): proof i has shape (n, m_i), m_i a power of
// two <= the verifier's m.  A key of length n m_i is a prefix of the verifier's key (PublicKey::new, publickey.rs:21-48;
// bpp_pk_hashed per index), and the window tables are stored per generator, so a prefix VIEW of the (n, m) tables
// serves (n, m_i): g, h and G_0.. sit where they sit, its H_i n (m - m_i) generators further on (VerifyShape::hgap).
// The pass gathers the caller-order records into one contiguous region per class (m_i), runs today's pass over each
// region with the class's view, and scatters the verdicts back into caller order.
#pragma once
#include <vector>

#include "host_util.hpp"

namespace bpp {

// one entry per proof, in caller order (built on the host, MX_WORDS 32-bit words): its first wire point and challenge
// in the caller's buffers and in the gathered regions, its position among the gathered proofs, its record and
// challenge-block lengths
enum { MX_PT = 0, MX_GPT, MX_CH, MX_GCH, MX_POS, MX_NV, MX_NCH, MX_WORDS = 8 };
constexpr unsigned MIXED_BLOCK = 128;
constexpr int MIXED_CLASSES = 8;   // m' = 1, 2, 4, .. <= VS_MAXM

// one block per proof: its NV wire points, its scalar triple and (ch != null) its 3 + k challenges, copied as 64-bit
// words by all the block's lanes (a (64,16) record on BLS12-381 is 507 words: four per lane)
template <class C>
__global__ void __launch_bounds__(MIXED_BLOCK) k_mixed_gather(const uint32_t* __restrict__ idx, size_t count,
                                                              const uint64_t* __restrict__ pts, const uint64_t* __restrict__ sc,
                                                              const uint64_t* __restrict__ ch, uint64_t* __restrict__ out_pts,
                                                              uint64_t* __restrict__ out_sc, uint64_t* __restrict__ out_ch) {
    constexpr uint32_t PW = C::Fp::N + 1;   // 64-bit words of a wire point
    const size_t i = blockIdx.x;
    if (i >= count) return;
    const uint32_t* e = idx + i * MX_WORDS;
    const uint64_t* src = pts + (size_t)e[MX_PT] * PW;
    uint64_t* dst = out_pts + (size_t)e[MX_GPT] * PW;
    const uint32_t words = e[MX_NV] * PW;
    for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) dst[w] = src[w];
    if (sc && threadIdx.x < 12) out_sc[(size_t)e[MX_POS] * 12 + threadIdx.x] = sc[i * 12 + threadIdx.x];
    if (ch) {
        const uint64_t* csrc = ch + (size_t)e[MX_CH] * 4;
        uint64_t* cdst = out_ch + (size_t)e[MX_GCH] * 4;
        for (uint32_t w = threadIdx.x; w < e[MX_NCH] * 4; w += blockDim.x) cdst[w] = csrc[w];
    }
}

// one wave per proof, four per block: from gathered position back to caller position -- the verdict (ok != null), the
// result point (res != null), the challenge block (ch != null)
template <class C>
__global__ void __launch_bounds__(256) k_mixed_scatter(const uint32_t* __restrict__ idx, size_t count,
                                                       const uint32_t* __restrict__ ok, const uint64_t* __restrict__ res,
                                                       const uint64_t* __restrict__ ch, uint32_t* __restrict__ out_ok,
                                                       uint64_t* __restrict__ out_res, uint64_t* __restrict__ out_ch) {
    constexpr uint32_t PW = C::Fp::N + 1;
    const size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= count) return;
    const uint32_t* e = idx + i * MX_WORDS;
    const size_t j = e[MX_POS];
    if (ok && lane == 0) out_ok[i] = ok[j];
    if (res)
        for (uint32_t w = lane; w < PW; w += 64) out_res[i * PW + w] = res[j * PW + w];
    if (ch) {
        const uint64_t* csrc = ch + (size_t)e[MX_GCH] * 4;
        uint64_t* cdst = out_ch + (size_t)e[MX_CH] * 4;
        for (uint32_t w = lane; w < e[MX_NCH] * 4; w += 64) cdst[w] = csrc[w];
    }
}

// The classes of a mixed batch.  Class c holds the proofs with m_i = 2^c, gathered in caller order behind the classes
// below it.  idx (when wanted): the per-proof entries k_mixed_gather / k_mixed_scatter read.
struct MixedPlan {
    size_t count[MIXED_CLASSES] = {}, first[MIXED_CLASSES] = {};   // proofs of the class, its first gathered position
    size_t pt[MIXED_CLASSES] = {}, chal[MIXED_CLASSES] = {};       // its first gathered wire point / challenge
    size_t points = 0, chals = 0;                                   // totals
    std::vector<uint32_t> idx;
};

// cap: the verifier's shape.  BPP_E_ARG (with the index of the first offending proof) for an m_i that is zero, not a power
// of two or larger than cap.m, or a batch whose wire points do not fit 32-bit offsets.
inline int mixed_plan(const VerifyShape& cap, const uint32_t* m_of, size_t count, bool want_idx, MixedPlan& p) {
    uint32_t logm = 0, logn = 0;
    while ((1u << logm) < cap.m) logm++;
    logn = cap.k - logm;
    auto nv = [&](uint32_t c) -> size_t { return 3 + 2 * (logn + c) + ((size_t)1 << c); };
    auto nch = [&](uint32_t c) -> size_t { return 3 + logn + c; };
    for (size_t i = 0; i < count; i++) {
        const uint32_t mi = m_of[i];
        if (mi == 0 || (mi & (mi - 1)) || mi > cap.m)
            return fail(BPP_E_ARG, "m_of[" + std::to_string(i) + "] = " + std::to_string(mi) +
                                       ": not a power of two in [1, " + std::to_string(cap.m) + "]");
        uint32_t c = 0;
        while ((1u << c) < mi) c++;
        p.count[c]++;
    }
    for (uint32_t c = 0; c < MIXED_CLASSES; c++) {
        p.first[c] = c ? p.first[c - 1] + p.count[c - 1] : 0;
        p.pt[c] = p.points;
        p.chal[c] = p.chals;
        p.points += p.count[c] * nv(c);
        p.chals += p.count[c] * nch(c);
    }
    if (p.points >= ((size_t)1 << 32) / 16) return fail(BPP_E_ARG, "count too large for one mixed batch");
    if (!want_idx) return BPP_OK;
    p.idx.assign(count * MX_WORDS, 0u);
    size_t next[MIXED_CLASSES];
    for (uint32_t c = 0; c < MIXED_CLASSES; c++) next[c] = p.first[c];
    size_t src_pt = 0, src_ch = 0;
    for (size_t i = 0; i < count; i++) {
        uint32_t c = 0;
        while ((1u << c) < m_of[i]) c++;
        const size_t pos = next[c]++, r = pos - p.first[c];
        uint32_t* e = p.idx.data() + i * MX_WORDS;
        e[MX_PT] = (uint32_t)src_pt;
        e[MX_GPT] = (uint32_t)(p.pt[c] + r * nv(c));
        e[MX_CH] = (uint32_t)src_ch;
        e[MX_GCH] = (uint32_t)(p.chal[c] + r * nch(c));
        e[MX_POS] = (uint32_t)pos;
        e[MX_NV] = (uint32_t)nv(c);
        e[MX_NCH] = (uint32_t)nch(c);
        src_pt += nv(c);
        src_ch += nch(c);
    }
    return BPP_OK;
}

}  // namespace bpp
