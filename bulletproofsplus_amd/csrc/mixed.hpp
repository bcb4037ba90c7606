// mixed.hpp -- batches of mixed aggregation sizes (bpp_verifier_run_mixed): proof i has shape (n, m_i), m_i a power of
// two <= the verifier's m.  A key of length n m_i is a prefix of the verifier's key (PublicKey::new, publickey.rs:21-48;
// bpp_pk_hashed per index), and the window tables are stored per generator, so a prefix VIEW of the (n, m) tables
// serves (n, m_i): g, h and G_0.. sit where they sit, its H_i n (m - m_i) generators further on (VerifyShape::hgap).
// The pass gathers the caller-order records into one contiguous region per class (m_i), runs today's pass over each
// region with the class's view, and scatters the verdicts back into caller order.
// Serialized form (bpp_range_verify_batch_serialized_mixed_device): the container decoder is the producer of the
// records, so it writes them straight into the class regions (k_container_decode_mixed) and nothing is gathered.
// Producing side (bpp_range_prove_batch_mixed_device, bpp_range_prove_batch_serialized_mixed_device): the same classes, each
// proved with its view; the prover writes every record once, through the per-proof index (prove_plan), into the caller-order
// packed block -- or into the class regions, from which k_container_encode_mixed writes the containers.
#pragma once
#include <vector>

#include "codec.hpp"
#include "host_util.hpp"
#include "outs_plan.hpp"
#include "prover_batch.hpp"

namespace bpp {

// one entry per proof, in caller order (built on the host, MX_WORDS 32-bit words): its first wire point and challenge
// in the caller's buffers and in the gathered regions, its position among the gathered proofs, its record and
// challenge-block lengths
enum { MX_PT = 0, MX_GPT, MX_CH, MX_GCH, MX_POS, MX_NV, MX_NCH, MX_WORDS = 8 };
constexpr unsigned MIXED_BLOCK = 128;
constexpr int MIXED_CLASSES = 8;   // m' = 1, 2, 4, .. <= VS_MAXM
static_assert(MIXED_CLASSES == OUTS_CLASSES, "outs_plan.hpp classes are the mixed classes");

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

// ---- serialized mixed batches: the decoder writes the class regions ------------------------------------------------
// one entry per proof, by GATHERED position (built on the host, SX_WORDS 32-bit words): the byte offsets of its container
// and of its commitments in the caller's packed buffers, and its caller position.  A RAGGED block (outs_of given, outs_plan.hpp:
// proof i covers outs_of[i] <= 2^c outputs, its other commitments are the identity and are not in the stream): SX_COMM is the
// ragged offset and SX_OUTS holds the count (outs_word); in any other block the kernels here leave that word unread, and
// the callers that scan or find put their own there (recover.hpp RX_BLIND).
enum { SX_PROOF = 0, SX_COMM, SX_CALLER, SX_OUTS, SX_WORDS = 4 };

// The class regions as the decode kernels see them, passed by value.  One lane per record point in gathered order; each
// class's lane range is padded to a multiple of the wave size, so a wave (= a block of these kernels) never straddles
// two classes and the class lookup below is wave-uniform.
struct SerClasses {
    uint32_t lane_end[MIXED_CLASSES];   // end of class c's padded lane range (cumulative, multiples of 64)
    uint32_t lanes[MIXED_CLASSES];      // lanes of the range in use: proofs of the class x NV(c)
    uint32_t first[MIXED_CLASSES];      // first gathered position of the class
    uint32_t pt[MIXED_CLASSES];         // first gathered record point of the class
    uint32_t n, logn;
    uint32_t ragged;                    // non-zero: SX_OUTS says how many of a proof's 2^c commitments the stream carries
};
constexpr uint32_t SER_WAVE = 64;
static_assert(SER_WAVE == OUTS_WAVE && CONTAINER_HDR == OUTS_HDR, "outs_plan.hpp mirrors the decoder's geometry");

// the commitments of the proof with index entry e that its stream carries; of the class's m the others are the identity
__device__ __forceinline__ uint32_t ser_outs(const SerClasses& g, const uint32_t* __restrict__ e, uint32_t m) {
    return g.ragged ? outs_word_count(e[SX_OUTS]) : m;
}
// the words the decoder writes for the encoding of the identity: the canonical infinity, on ristretto255 the
// representative (0, 1) that rist_decode gives for 32 zero bytes
template <class C>
__device__ __forceinline__ void record_identity(uint32_t* __restrict__ w) {
    constexpr int N = C::Fp::N;
#pragma unroll
    for (int t = 0; t < 2 * N + 2; t++) w[t] = 0;
    w[C::ID == 2 ? N : 2 * N] = 1;
}

// a lane of the serialized mixed kernels: its class's shape (n, m, k, NV), the proof's gathered position, the point's
// index in the record and among the gathered points; `live` false for a padding lane
struct SerLane {
    uint32_t m, k, NV, pos, t, point;
    bool live;
};
// base: the wave's first lane (wave-uniform, so the comparisons and selects below are scalar work)
__device__ __forceinline__ SerLane ser_lane(const SerClasses& g, uint32_t base, uint32_t lane_in_wave) {
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < MIXED_CLASSES - 1; j++) c += base >= g.lane_end[j] ? 1u : 0u;   // empty classes are skipped
    uint32_t start = 0, lanes = 0, first = 0, pt = 0;
#pragma unroll
    for (int j = 0; j < MIXED_CLASSES; j++)
        if ((uint32_t)j == c) {
            start = j ? g.lane_end[j - 1] : 0u;
            lanes = g.lanes[j];
            first = g.first[j];
            pt = g.pt[j];
        }
    SerLane L;
    L.m = 1u << c;
    L.k = g.logn + c;
    L.NV = 3 + 2 * L.k + L.m;
    const uint32_t j = base - start + lane_in_wave;
    L.live = j < lanes;
    const uint32_t r = j / L.NV;
    L.pos = first + r;
    L.t = j - r * L.NV;
    L.point = pt + j;
    return L;
}

// k_container_decode over a mixed batch: one lane per record point of all classes in gathered order.  The containers are
// read where the caller packed them (idx: SX_PROOF / SX_COMM, lengths implied by m_of on the host, never by the bytes)
// and decoded straight into the class regions; status words by gathered position.  A commitment lane beyond the proof's
// count (a ragged block) reads no byte and writes the identity's record words.
template <class C>
__global__ void __launch_bounds__(64, 2) k_container_decode_mixed(SerClasses g, const uint32_t* __restrict__ idx,
                                                                  const uint8_t* __restrict__ proofs,
                                                                  const uint8_t* __restrict__ commitments,
                                                                  uint32_t* __restrict__ records, uint32_t* __restrict__ scalars,
                                                                  uint32_t* __restrict__ status, uint32_t version) {
    constexpr int N = C::Fp::N;
    const SerLane L = ser_lane(g, blockIdx.x * SER_WAVE, threadIdx.x);
    if (!L.live) return;
    const int CB = container_point_bytes<C>(version);
    const uint32_t* e = idx + (size_t)L.pos * SX_WORDS;
    const uint32_t npp = 3 + 2 * L.k;
    uint32_t* w = records + (size_t)L.point * (2 * N + 2);
    if (L.t >= npp + ser_outs(g, e, L.m)) {
        record_identity<C>(w);
        return;
    }
    const uint8_t* rec = proofs + e[SX_PROOF];
    const uint8_t* src = L.t < npp ? rec + CONTAINER_HDR + (size_t)L.t * CB : commitments + e[SX_COMM] + (size_t)(L.t - npp) * CB;
    if (!container_decode_lane<C>(rec, src, L.t, g.n, L.m, L.k, version, w, scalars + (size_t)L.pos * 24))
        atomicOr(status + L.pos, 1u);
}

// The decoder's mirror (bpp_range_prove_batch_serialized_mixed_device): one lane per record point of all classes in gathered
// order encodes its point out of the class regions -- lane t < 3 + 2k into container SX_PROOF at CONTAINER_HDR + t CB, the
// others as commitment t - (3 + 2k) at SX_COMM -- and the lane of a proof's first point writes the 12-byte header and the
// three scalars (scalars: by CALLER position, as k_pb_final leaves them for a mixed block).  Byte stores throughout: a
// container starts wherever the ones before it end (a secp256k1 point is 33 bytes), and a lane's bytes are its own.
// A commitment lane beyond the proof's count (a ragged block) writes nothing: its point is the identity by construction.
template <class C>
__global__ void __launch_bounds__(64, 2) k_container_encode_mixed(SerClasses g, const uint32_t* __restrict__ idx,
                                                                  const uint32_t* __restrict__ records,
                                                                  const uint32_t* __restrict__ scalars,
                                                                  uint8_t* __restrict__ proofs, uint8_t* __restrict__ commitments,
                                                                  uint32_t version) {
    constexpr int N = C::Fp::N;
    const SerLane L = ser_lane(g, blockIdx.x * SER_WAVE, threadIdx.x);
    if (!L.live) return;
    const int CB = container_point_bytes<C>(version);
    const uint32_t* e = idx + (size_t)L.pos * SX_WORDS;
    const uint32_t npp = 3 + 2 * L.k;
    if (L.t >= npp + ser_outs(g, e, L.m)) return;
    uint8_t* rec = proofs + e[SX_PROOF];
    uint8_t* dst = L.t < npp ? rec + CONTAINER_HDR + (size_t)L.t * CB : commitments + e[SX_COMM] + (size_t)(L.t - npp) * CB;
    const uint32_t* w = records + (size_t)L.point * (2 * N + 2);
    if (version == 2) point_uncompressed_write<C>(w, dst);
    else point_compress<C>(w, dst);
    if (L.t == 0) {
        const uint8_t hdr[CONTAINER_HDR] = {'B', 'P', 'P', '+', (uint8_t)version, (uint8_t)C::ID, (uint8_t)g.n, (uint8_t)L.m, (uint8_t)L.k, 0, 0, 0};
        for (uint32_t b = 0; b < CONTAINER_HDR; b++) rec[b] = hdr[b];
        uint8_t* sc = rec + CONTAINER_HDR + (size_t)npp * CB;
        const uint32_t* sw = scalars + (size_t)e[SX_CALLER] * 24;
        for (int q = 0; q < 24; q++) {
            const uint32_t v = sw[q];
            sc[4 * q] = (uint8_t)v;
            sc[4 * q + 1] = (uint8_t)(v >> 8);
            sc[4 * q + 2] = (uint8_t)(v >> 16);
            sc[4 * q + 3] = (uint8_t)(v >> 24);
        }
    }
}

// k_records_subgroup over the class regions (same lanes as k_container_decode_mixed): one launch for all classes.  The
// padded lanes of a ragged block hold the infinity the decoder wrote: record_leaves_subgroup ends on its flag word.
template <class C>
__global__ void __launch_bounds__(64, 2) k_records_subgroup_mixed(SerClasses g, uint32_t* __restrict__ records,
                                                                  uint32_t* __restrict__ status) {
    constexpr int N = C::Fp::N;
    const SerLane L = ser_lane(g, blockIdx.x * SER_WAVE, threadIdx.x);
    if (!L.live) return;
    if (record_leaves_subgroup<C>(records + (size_t)L.point * (2 * N + 2))) atomicOr(status + L.pos, 1u);
}

// k_container_status and the scatter in one: out_ok[caller position] = FormatError where the decoder rejected the proof,
// else the pass's verdict
template <class C>
__global__ void __launch_bounds__(256) k_mixed_status_scatter(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ status,
                                                              const uint32_t* __restrict__ ok, uint32_t* __restrict__ out_ok,
                                                              size_t count) {
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= count) return;
    out_ok[idx[pos * SX_WORDS + SX_CALLER]] = status[pos] ? (uint32_t)BPP_FORMAT_ERROR : ok[pos];
}

// The classes of a mixed batch.  Class c holds the proofs with m_i = 2^c, gathered in caller order behind the classes
// below it.  idx (when wanted): the per-proof entries k_mixed_gather / k_mixed_scatter read.
struct MixedPlan {
    size_t count[MIXED_CLASSES] = {}, first[MIXED_CLASSES] = {};   // proofs of the class, its first gathered position
    size_t pt[MIXED_CLASSES] = {}, chal[MIXED_CLASSES] = {};       // its first gathered wire point / challenge
    size_t points = 0, chals = 0;                                   // totals
    std::vector<uint32_t> idx;
    // serialized form (mixed_plan_serialized): the packed input's sizes, the per-proof entries by gathered position
    // (SX_*), the lane ranges of the decode kernels
    size_t proof_bytes = 0, comm_bytes = 0, lanes = 0;
    size_t n_out = 0;   // commitments the stream carries: the sum of m_i, of a ragged block the sum of outs_of[i]
    std::vector<uint32_t> sidx;
    SerClasses classes = {};
    // producing side (prove_plan): the prover's per-proof entries by gathered position (PX_*, prover_batch.hpp)
    std::vector<uint32_t> px;
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

// mixed_plan for containers packed back to back in caller order (container i of hdr + (3 + 2 k_i) pb + 96 bytes, then
// m_i encoded commitments of pb bytes each in a buffer of their own).  pb: bytes of an encoded point.  BPP_E_ARG also
// for a batch whose byte offsets do not fit the 32-bit index.
// outs_of given (m_of is then not read): a ragged block -- proof i has the shape of its class, m_i = 2^ceil(log2 outs_of[i]),
// and outs_of[i] commitments in the stream (outs_plan.hpp, whose errors name outs_of[i]).
inline int mixed_plan_serialized(const VerifyShape& cap, const uint32_t* m_of, size_t count, size_t pb, bool want_idx,
                                 MixedPlan& p, const uint32_t* outs_of = nullptr) {
    OutsPlan ragged;
    if (outs_of) {
        if (int rc = outs_plan(cap.n, cap.m, outs_of, count, pb, ragged)) return rc;
        m_of = ragged.m_of.data();
    }
    int rc = mixed_plan(cap, m_of, count, false, p);
    if (rc) return rc;
    uint32_t logm = 0;
    while ((1u << logm) < cap.m) logm++;
    const uint32_t logn = cap.k - logm;
    auto nv = [&](uint32_t c) -> size_t { return 3 + 2 * (logn + c) + ((size_t)1 << c); };
    auto cbytes = [&](uint32_t c) -> size_t { return CONTAINER_HDR + (size_t)(3 + 2 * (logn + c)) * pb + 96; };
    SerClasses& g = p.classes;
    g.n = cap.n;
    g.logn = logn;
    size_t lanes = 0;
    for (uint32_t c = 0; c < MIXED_CLASSES; c++) {
        p.proof_bytes += p.count[c] * cbytes(c);
        p.n_out += p.count[c] << c;
        const size_t used = p.count[c] * nv(c);   // < 2^28 in all (mixed_plan)
        lanes += (used + SER_WAVE - 1) / SER_WAVE * SER_WAVE;
        g.lane_end[c] = (uint32_t)lanes;
        g.lanes[c] = (uint32_t)used;
        g.first[c] = (uint32_t)p.first[c];
        g.pt[c] = (uint32_t)p.pt[c];
    }
    p.lanes = lanes;
    g.ragged = outs_of ? 1u : 0u;
    if (outs_of) p.n_out = ragged.n_out;
    p.comm_bytes = p.n_out * pb;
    if ((p.proof_bytes | p.comm_bytes) >> 32) {   // name the first proof that ends beyond 4 GiB (ragged: outs_plan has)
        size_t i = 0;
        for (size_t pr = 0, cm = 0; i < count; i++) {
            const uint32_t c = (uint32_t)__builtin_ctz(m_of[i]);
            pr += cbytes(c);
            cm += ((size_t)1 << c) * pb;
            if ((pr | cm) >> 32) break;
        }
        return fail(BPP_E_ARG, "batch too large: the bytes of m_of[" + std::to_string(i) + "] lie beyond the 32-bit index");
    }
    if (!want_idx) return BPP_OK;
    p.sidx.assign(count * SX_WORDS, 0u);
    size_t next[MIXED_CLASSES];
    for (uint32_t c = 0; c < MIXED_CLASSES; c++) next[c] = p.first[c];
    size_t src_pr = 0, src_cm = 0;
    for (size_t i = 0; i < count; i++) {
        uint32_t c = 0;
        while ((1u << c) < m_of[i]) c++;
        uint32_t* e = p.sidx.data() + next[c]++ * SX_WORDS;
        e[SX_PROOF] = (uint32_t)src_pr;
        e[SX_COMM] = (uint32_t)src_cm;
        e[SX_CALLER] = (uint32_t)i;
        if (outs_of) e[SX_OUTS] = outs_word(outs_of[i], 0);
        src_pr += cbytes(c);
        src_cm += (outs_of ? (size_t)outs_of[i] : (size_t)1 << c) * pb;
    }
    return BPP_OK;
}

// The plan of a block to PROVE: mixed_plan / mixed_plan_serialized (pb != 0: the containers' point size) and the prover's
// index px by gathered position.  PX_REC: wire form -- the proof's record in the caller-order packed block (what
// bpp_verifier_run_mixed reads as d_points); serialized form -- its record in the class regions.
// outs_of given (serialized form alone; m_of is then not read): a ragged block -- PX_VAL is the ragged offset, PX_OUTS the count.
inline int prove_plan(const VerifyShape& cap, const uint32_t* m_of, size_t count, size_t pb, bool want_idx, MixedPlan& p,
                      const uint32_t* outs_of = nullptr) {
    if (outs_of && !pb) return fail(BPP_E_ARG, "outs_of: the serialized form alone");
    int rc = pb ? mixed_plan_serialized(cap, m_of, count, pb, want_idx, p, outs_of) : mixed_plan(cap, m_of, count, false, p);
    if (rc || !want_idx) return rc;
    uint32_t logm = 0;
    while ((1u << logm) < cap.m) logm++;
    const uint32_t logn = cap.k - logm;
    p.px.assign(count * PX_WORDS, 0u);
    size_t next[MIXED_CLASSES];
    for (uint32_t c = 0; c < MIXED_CLASSES; c++) next[c] = p.first[c];
    size_t src_pt = 0, src_val = 0, src_bl = 0, src_ch = 0;
    for (size_t i = 0; i < count; i++) {
        const uint32_t c = outs_class(outs_of ? outs_of[i] : m_of[i]);
        const uint32_t k = logn + c;
        const size_t nv = 3 + 2 * (size_t)k + ((size_t)1 << c);
        const size_t pos = next[c]++;
        uint32_t* e = p.px.data() + pos * PX_WORDS;
        e[PX_REC] = (uint32_t)(pb ? p.pt[c] + (pos - p.first[c]) * nv : src_pt);
        e[PX_CALLER] = (uint32_t)i;
        e[PX_VAL] = (uint32_t)src_val;
        e[PX_BLIND] = (uint32_t)src_bl;
        e[PX_CH] = (uint32_t)src_ch;
        e[PX_OUTS] = outs_of ? outs_of[i] : 1u << c;
        src_pt += nv;
        src_val += e[PX_OUTS];
        src_bl += pb_blind_elems(k);
        src_ch += 3 + k;
    }
    return BPP_OK;
}

}  // namespace bpp
