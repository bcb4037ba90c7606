// bpp_amd.hpp -- C++ host-side mirror of the reference crate's API for the hot path, over the C ABI of
// bpp_amd.h (header only; link with -lbpp_amd).  The reference is Rust; no Rust toolchain exists in the
// build image, so the host side above the C ABI is C++ with the reference's names, argument meaning and
// error behaviour (paths relative to /root/reference/src):
//
//   bpp::Arith::init()                         bls12_381/building_block/arith.rs:6-19
//   bpp::PrimeFieldElem                        bls12_381/building_block/scalar/prime_field_elem.rs:13-15 (as data)
//   bpp::Point                                 bls12_381/building_block/point/point.rs:12 (as data, wire format)
//   bpp::MulVec                                bls12_381/building_block/mulvec.rs:7-53
//   bpp::PublicKey{g,h,G_vec,H_vec}            publickey.rs:13-52
//   bpp::RangeProver{v_vec,gamma_vec,commitment_vec}   range/prover.rs:13-42
//   bpp::RangeVerifier{commitment_vec}.allocate()       README.md:47-48 (no code in the reference)
//   bpp::WeightedInnerProductProof::prove / verify      weighted_inner_product_proof.rs:25-33, :36-227, :238-328
//   bpp::RangeProof{A, proof}::prove / verify  range/mod.rs:25-78
//   bpp::ProofError::VerificationError         errors.rs:14-50
//
// Where the reference panics (assert!/panic!) these classes throw std::logic_error; `verify` returns
// Result-like `std::optional<ProofError>` (nullopt = Ok(())).  Every operation runs HIP kernels through
// libbpp_amd.so; nothing here computes on the CPU beyond (de)serialisation.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "bpp_amd.h"

namespace bpp {

enum class ProofError { VerificationError };

// One process-wide context per curve, as the reference's global Once-guarded init.
class Arith {
  public:
    static void init(int curve_id = BPP_BLS12_381_G1, int device = 0) {
        std::lock_guard<std::mutex> lk(mu());
        if (ctx_ref()) return;
        bpp_ctx* c = nullptr;
        if (bpp_init(curve_id, device, &c) != BPP_OK)
            throw std::runtime_error(std::string("Initializing bpp_amd failed: ") + bpp_last_error());  // arith.rs:13-15
        ctx_ref() = c;
        curve_ref() = curve_id;
    }
    static bpp_ctx* ctx() {
        if (!ctx_ref()) init();
        return ctx_ref();
    }
    static int curve() { return curve_ref(); }
    static size_t point_words() { return (size_t)bpp_point_words(curve_ref()); }

  private:
    static bpp_ctx*& ctx_ref() {
        static bpp_ctx* c = nullptr;
        return c;
    }
    static int& curve_ref() {
        static int c = BPP_BLS12_381_G1;
        return c;
    }
    static std::mutex& mu() {
        static std::mutex m;
        return m;
    }
};

// canonical value < r as 4 little-endian u64 limbs
struct PrimeFieldElem {
    std::array<uint64_t, 4> e{};
    PrimeFieldElem() = default;
    // PrimeFieldElem::new(i32) for n >= 0 (negative values need the group order: use from_limbs)
    explicit PrimeFieldElem(uint32_t n) { e[0] = n; }
    static PrimeFieldElem from_limbs(const uint64_t* l) {
        PrimeFieldElem x;
        std::memcpy(x.e.data(), l, 32);
        return x;
    }
    bool operator==(const PrimeFieldElem& o) const { return e == o.e; }
};

// affine wire point: x | y | inf  (2L+1 u64 words)
struct Point {
    std::vector<uint64_t> w;
    Point() : w(Arith::point_words(), 0) { w.back() = 1; }   // Point::zero()
    explicit Point(const uint64_t* src) : w(src, src + Arith::point_words()) {}
    static Point zero() { return Point(); }
    bool is_zero() const { return w.back() != 0; }
    bool operator==(const Point& o) const { return w == o.w; }
};

class MulVec {
  public:
    void add_scalar(const PrimeFieldElem& s) { scalars_.insert(scalars_.end(), s.e.begin(), s.e.end()); n_s_++; }
    void add_scalars(const std::vector<PrimeFieldElem>& ss) { for (auto& s : ss) add_scalar(s); }
    void add_point(const Point& p) { points_.insert(points_.end(), p.w.begin(), p.w.end()); n_p_++; }
    void add_points(const std::vector<Point>& ps) { for (auto& p : ps) add_point(p); }
    Point calculate() const {
        if (n_s_ != n_p_) throw std::logic_error("mulvec: lengths of scalars and points must match");  // mulvec.rs:23-25
        Point out;
        int rc = bpp_msm(Arith::ctx(), scalars_.data(), points_.data(), n_s_, out.w.data());
        if (rc != BPP_OK) throw std::runtime_error(std::string("bpp_msm: ") + bpp_last_error());
        return out;
    }

  private:
    std::vector<uint64_t> scalars_, points_;
    size_t n_s_ = 0, n_p_ = 0;
};

struct PublicKey {
    Point g, h;
    std::vector<Point> G_vec, H_vec;
    static PublicKey create(size_t length) {   // PublicKey::new(length), publickey.rs:21-48
        const size_t pw = Arith::point_words();
        std::vector<uint64_t> gh(2 * pw), G(length * pw + 1), H(length * pw + 1);
        if (bpp_pk_new(Arith::ctx(), length, gh.data(), G.data(), H.data()) != BPP_OK)
            throw std::runtime_error(std::string("bpp_pk_new: ") + bpp_last_error());
        PublicKey pk;
        pk.g = Point(gh.data());
        pk.h = Point(gh.data() + pw);
        for (size_t i = 0; i < length; i++) {
            pk.G_vec.emplace_back(G.data() + i * pw);
            pk.H_vec.emplace_back(H.data() + i * pw);
        }
        return pk;
    }
    Point commitment(const PrimeFieldElem& v, const PrimeFieldElem& gamma) const {   // publickey.rs:50-52
        MulVec mv;
        mv.add_scalar(v);
        mv.add_scalar(gamma);
        mv.add_point(g);
        mv.add_point(h);
        return mv.calculate();
    }
    std::vector<uint64_t> gh_wire() const {
        std::vector<uint64_t> o(g.w);
        o.insert(o.end(), h.w.begin(), h.w.end());
        return o;
    }
    static std::vector<uint64_t> flat(const std::vector<Point>& v) {
        std::vector<uint64_t> o;
        for (auto& p : v) o.insert(o.end(), p.w.begin(), p.w.end());
        return o;
    }
};

struct RangeProver {
    std::vector<uint64_t> v_vec;
    std::vector<PrimeFieldElem> gamma_vec;
    std::vector<Point> commitment_vec;
    // range/prover.rs:28-42.  amount64 = false keeps the `v as i32` of prover.rs:37; true commits the whole 64-bit amount,
    // V = v g + gamma h (a two-term MulVec): the commitment a proof made under BPP_PROVE_AMOUNT64 verifies against
    void commit(const PublicKey& pk, uint64_t v, const PrimeFieldElem& gamma, bool amount64 = false) {
        Point out;
        if (amount64) {
            PrimeFieldElem s;
            s.e[0] = v;
            out = pk.commitment(s, gamma);
        } else {
            auto gh = pk.gh_wire();
            if (bpp_commit(Arith::ctx(), gh.data(), v, gamma.e.data(), out.w.data()) != BPP_OK)
                throw std::runtime_error(std::string("bpp_commit: ") + bpp_last_error());
        }
        v_vec.push_back(v);
        gamma_vec.push_back(gamma);
        commitment_vec.push_back(out);
    }
};

// RangeProver::commit (range/prover.rs:28-42) for a block of values over an engine's g and h, through its window tables
// (bpp_commit_batch): amount64 = false keeps the `v as i32` of prover.rs:37, true (BPP_PROVE_AMOUNT64) commits the whole u64
inline std::vector<Point> commit_batch(bpp_verifier* engine, const std::vector<uint64_t>& values,
                                       const std::vector<PrimeFieldElem>& gammas, bool amount64 = false) {
    if (values.size() != gammas.size()) throw std::logic_error("commit_batch: one gamma per value");
    const size_t pw = Arith::point_words();
    std::vector<uint64_t> gw, out(values.size() * pw + 1);
    for (auto& g : gammas) gw.insert(gw.end(), g.e.begin(), g.e.end());
    if (bpp_commit_batch(engine, values.data(), gw.data(), values.size(), amount64 ? BPP_PROVE_AMOUNT64 : 0, out.data()) != BPP_OK)
        throw std::runtime_error(std::string("bpp_commit_batch: ") + bpp_last_error());
    std::vector<Point> V;
    for (size_t i = 0; i < values.size(); i++) V.emplace_back(out.data() + i * pw);
    return V;
}

// Mask recovery from wire data (bpp_range_recover_masks_mixed): Gamma_i = gamma_0 + z^2 gamma_1 + .. of proof i from its
// scalar triple [r', s', delta'], its challenge block (`challenges`: the 3 + k_i scalars of every proof back to back, or empty
// for the reference's literals) and the blinding key it was made under; `index` names each proof's blinding index (empty:
// index_base + i).  For ms[i] = 1 Gamma_i is the output's mask.  NOT a verification; key and index together are a view key.
inline std::vector<PrimeFieldElem> recover_masks(bpp_verifier* engine, const std::vector<PrimeFieldElem>& scalars,
                                                 const std::vector<uint32_t>& ms, const std::vector<PrimeFieldElem>& challenges,
                                                 const std::array<uint8_t, 32>& blind_key, uint64_t index_base = 0,
                                                 const std::vector<uint64_t>& index = {}) {
    if (scalars.size() != 3 * ms.size()) throw std::logic_error("recover_masks: three scalars per proof");
    if (!index.empty() && index.size() != ms.size()) throw std::logic_error("recover_masks: one index per proof");
    std::vector<uint64_t> sw, cw, out(ms.size() * 4 + 1);
    for (auto& s : scalars) sw.insert(sw.end(), s.e.begin(), s.e.end());
    for (auto& c : challenges) cw.insert(cw.end(), c.e.begin(), c.e.end());
    if (bpp_range_recover_masks_mixed(engine, sw.data(), ms.data(), ms.size(), cw.empty() ? nullptr : cw.data(), blind_key.data(),
                                      index_base, index.empty() ? nullptr : index.data(), nullptr, out.data()) != BPP_OK)
        throw std::runtime_error(std::string("bpp_range_recover_masks_mixed: ") + bpp_last_error());
    std::vector<PrimeFieldElem> masks(ms.size());
    for (size_t i = 0; i < ms.size(); i++)
        for (int t = 0; t < 4; t++) masks[i].e[t] = out[i * 4 + t];
    return masks;
}

// Scanning a block of serialized proofs made under the transcript for the outputs of a blinding key
// (bpp_range_scan_serialized_mixed): proofs, commitments and ms as bpp_range_verify_batch_serialized_mixed takes them;
// `amounts` one candidate amount per proof, read for ms[i] = 1 (empty: nothing is confirmed); amount64: the proofs commit
// whole u64 amounts.  status[i]: 0 the output opens to (amount, Gamma) -- it is the key's, Gamma its mask; 1 it does not (Gamma
// zero); 2 FormatError (Gamma zero); BPP_SCAN_UNCONFIRMED no amount or ms[i] > 1.  A scan is NOT a verification.
struct ScanResult {
    std::vector<uint32_t> status;
    std::vector<PrimeFieldElem> masks;
};
inline ScanResult scan_serialized_mixed(bpp_verifier* engine, const std::vector<uint8_t>& proofs,
                                        const std::vector<uint8_t>& commitments, const std::vector<uint32_t>& ms,
                                        const std::array<uint8_t, 32>& blind_key, uint64_t index_base = 0,
                                        const std::vector<uint64_t>& index = {}, const std::vector<uint64_t>& amounts = {},
                                        bool amount64 = false, bool uncompressed = false) {
    if (!index.empty() && index.size() != ms.size()) throw std::logic_error("scan_serialized_mixed: one index per proof");
    if (!amounts.empty() && amounts.size() != ms.size()) throw std::logic_error("scan_serialized_mixed: one amount per proof");
    ScanResult r;
    r.status.assign(ms.size() + 1, 0);
    std::vector<uint64_t> out(ms.size() * 4 + 1);
    const int flags = BPP_SER_TRANSCRIPT | (uncompressed ? BPP_SER_UNCOMPRESSED : 0) | (amount64 ? BPP_PROVE_AMOUNT64 : 0);
    if (bpp_range_scan_serialized_mixed(engine, proofs.data(), commitments.data(), ms.data(), ms.size(), flags, blind_key.data(),
                                        index_base, index.empty() ? nullptr : index.data(), nullptr,
                                        amounts.empty() ? nullptr : amounts.data(), out.data(), r.status.data()) != BPP_OK)
        throw std::runtime_error(std::string("bpp_range_scan_serialized_mixed: ") + bpp_last_error());
    r.status.resize(ms.size());
    r.masks.resize(ms.size());
    for (size_t i = 0; i < ms.size(); i++)
        for (int t = 0; t < 4; t++) r.masks[i].e[t] = out[i * 4 + t];
    return r;
}

// The same scan under MANY keys in one call (bpp_range_scan_serialized_mixed_keys): the decode, the membership test, the
// challenges and the inversions run once, the key-dependent part per (key, proof) pair.  The blinding index of proof i
// (index[i], or index_base + i) is shared by all keys; `amounts` is key-major, keys.size() x ms.size() (empty: nothing is
// confirmed).  Result: key-major, pair (j, i) at j * ms.size() + i, the status words of scan_serialized_mixed.  Every key
// is a view key; a scan is NOT a verification.
inline ScanResult scan_serialized_mixed_keys(bpp_verifier* engine, const std::vector<uint8_t>& proofs,
                                             const std::vector<uint8_t>& commitments, const std::vector<uint32_t>& ms,
                                             const std::vector<std::array<uint8_t, 32>>& keys, uint64_t index_base = 0,
                                             const std::vector<uint64_t>& index = {}, const std::vector<uint64_t>& amounts = {},
                                             bool amount64 = false, bool uncompressed = false) {
    const size_t pairs = keys.size() * ms.size();
    if (!index.empty() && index.size() != ms.size()) throw std::logic_error("scan_serialized_mixed_keys: one index per proof");
    if (!amounts.empty() && amounts.size() != pairs) throw std::logic_error("scan_serialized_mixed_keys: K x count amounts");
    ScanResult r;
    r.status.assign(pairs + 1, 0);
    std::vector<uint64_t> out(pairs * 4 + 1);
    std::vector<uint8_t> packed(keys.size() * 32 + 1);
    for (size_t j = 0; j < keys.size(); j++)
        for (size_t t = 0; t < 32; t++) packed[j * 32 + t] = keys[j][t];
    const int flags = BPP_SER_TRANSCRIPT | (uncompressed ? BPP_SER_UNCOMPRESSED : 0) | (amount64 ? BPP_PROVE_AMOUNT64 : 0);
    const int rc = bpp_range_scan_serialized_mixed_keys(engine, proofs.data(), commitments.data(), ms.data(), ms.size(), flags,
                                                        packed.data(), keys.size(), index_base,
                                                        index.empty() ? nullptr : index.data(),
                                                        amounts.empty() ? nullptr : amounts.data(), out.data(), r.status.data());
    for (volatile uint8_t& b : packed) b = 0;   // the packed copy of the keys made here
    if (rc != BPP_OK) throw std::runtime_error(std::string("bpp_range_scan_serialized_mixed_keys: ") + bpp_last_error());
    r.status.resize(pairs);
    r.masks.resize(pairs);
    for (size_t i = 0; i < pairs; i++)
        for (int t = 0; t < 4; t++) r.masks[i].e[t] = out[i * 4 + t];
    return r;
}

// amount XOR pad(blind_key, index) per amount (bpp_amounts_seal): seals amounts, and opens sealed ones.  The index of amount
// i is index[i], or index_base + i: the blinding index of the output's proof.
inline std::vector<uint64_t> seal_amounts(bpp_ctx* ctx, const std::array<uint8_t, 32>& blind_key,
                                          const std::vector<uint64_t>& amounts, uint64_t index_base = 0,
                                          const std::vector<uint64_t>& index = {}) {
    if (!index.empty() && index.size() != amounts.size()) throw std::logic_error("seal_amounts: one index per amount");
    std::vector<uint64_t> out(amounts.size() + 1);
    if (bpp_amounts_seal(ctx, blind_key.data(), index_base, index.empty() ? nullptr : index.data(), amounts.data(), amounts.size(),
                         out.data()) != BPP_OK)
        throw std::runtime_error(std::string("bpp_amounts_seal: ") + bpp_last_error());
    out.resize(amounts.size());
    return out;
}

// Verifying a block AND listing the single outputs that belong to `keys` in one call, the common front of
// bpp_range_verify_batch_serialized_mixed and scan_serialized_mixed_keys run once
// (bpp_range_verify_find_serialized_mixed_keys).  `amounts`: sealed -- one sealed amount per proof, shared by all keys; else
// key-major, keys.size() x ms.size() candidates.  ok[i]: the verdict of proof i under the transcript, 0 / 1 / 2.  hits: in
// ascending (key number, position), at most max_hits of them; found: how many there are.  A hit is a VERIFIED single output
// whose commitment opens to the amount and the mask recovered under that key.  Every key is a view key.  With no keys the
// block is verified all the same (ok is the library's in every case, never a default).
struct FindHit {
    uint32_t key_no, position;
    uint64_t amount;
    PrimeFieldElem mask;
};
struct FindResult {
    std::vector<uint32_t> ok;
    std::vector<FindHit> hits;
    size_t found;
};
inline FindResult verify_find_serialized_mixed_keys(bpp_verifier* engine, const std::vector<uint8_t>& proofs,
                                                    const std::vector<uint8_t>& commitments, const std::vector<uint32_t>& ms,
                                                    const std::vector<std::array<uint8_t, 32>>& keys,
                                                    const std::vector<uint64_t>& amounts, bool sealed, size_t max_hits,
                                                    uint64_t index_base = 0, const std::vector<uint64_t>& index = {},
                                                    bool amount64 = false, bool uncompressed = false) {
    const size_t pairs = keys.size() * ms.size();
    if (!index.empty() && index.size() != ms.size()) throw std::logic_error("verify_find_serialized_mixed_keys: one index per proof");
    if (amounts.size() != (sealed ? ms.size() : pairs))
        throw std::logic_error("verify_find_serialized_mixed_keys: one sealed amount per proof, or K x count amounts");
    const size_t cap = std::min(max_hits, pairs);
    FindResult r;
    r.ok.assign(ms.size() + 1, 0);
    std::vector<uint32_t> rec(cap * 12 + 1);
    std::vector<uint8_t> packed(keys.size() * 32 + 1);
    for (size_t j = 0; j < keys.size(); j++)
        for (size_t t = 0; t < 32; t++) packed[j * 32 + t] = keys[j][t];
    const int flags = BPP_SER_TRANSCRIPT | (uncompressed ? BPP_SER_UNCOMPRESSED : 0) | (amount64 ? BPP_PROVE_AMOUNT64 : 0) |
                      (sealed ? BPP_FIND_AMOUNTS_SEALED : 0);
    uint32_t found = 0;
    const int rc = bpp_range_verify_find_serialized_mixed_keys(engine, proofs.data(), commitments.data(), ms.data(), ms.size(),
                                                               flags, packed.data(), keys.size(), index_base,
                                                               index.empty() ? nullptr : index.data(), amounts.data(),
                                                               r.ok.data(), rec.data(), cap, &found);
    for (volatile uint8_t& b : packed) b = 0;   // the packed copy of the keys made here
    if (rc != BPP_OK) throw std::runtime_error(std::string("bpp_range_verify_find_serialized_mixed_keys: ") + bpp_last_error());
    r.ok.resize(ms.size());
    r.found = found;
    r.hits.resize(std::min<size_t>(found, cap));
    for (size_t h = 0; h < r.hits.size(); h++) {
        const uint32_t* w = rec.data() + h * 12;
        r.hits[h].key_no = w[0];
        r.hits[h].position = w[1];
        r.hits[h].amount = (uint64_t)w[2] | (uint64_t)w[3] << 32;
        for (int t = 0; t < 4; t++) r.hits[h].mask.e[t] = (uint64_t)w[4 + 2 * t] | (uint64_t)w[5 + 2 * t] << 32;
    }
    return r;
}

// view_tag(blind_key, index) per output (bpp_view_tags): the byte a SENDER attaches to an output next to its sealed amount.
// The index of output i is index[i], or index_base + i.  The tag authenticates nothing.
inline std::vector<uint8_t> view_tags(bpp_ctx* ctx, const std::array<uint8_t, 32>& blind_key, size_t count, uint64_t index_base = 0,
                                      const std::vector<uint64_t>& index = {}) {
    if (!index.empty() && index.size() != count) throw std::logic_error("view_tags: one index per output");
    std::vector<uint8_t> out(count + 1);
    if (bpp_view_tags(ctx, blind_key.data(), index_base, index.empty() ? nullptr : index.data(), count, out.data()) != BPP_OK)
        throw std::runtime_error(std::string("bpp_view_tags: ") + bpp_last_error());
    out.resize(count);
    return out;
}

// verify_find_serialized_mixed_keys with the outputs' view tags (bpp_range_verify_find_tagged_serialized_mixed_keys): `tags`
// holds one byte per proof, shared by all keys; a pair whose tag does not match its key is ruled out after one hash.  ok
// is the untagged call's; the hits are its hits among the candidates; candidates: the pairs that passed the tag test.
struct FindTaggedResult {
    std::vector<uint32_t> ok;
    std::vector<FindHit> hits;
    size_t found, candidates;
};
inline FindTaggedResult verify_find_tagged_serialized_mixed_keys(
    bpp_verifier* engine, const std::vector<uint8_t>& proofs, const std::vector<uint8_t>& commitments,
    const std::vector<uint32_t>& ms, const std::vector<std::array<uint8_t, 32>>& keys, const std::vector<uint64_t>& amounts,
    bool sealed, const std::vector<uint8_t>& tags, size_t max_hits, uint64_t index_base = 0,
    const std::vector<uint64_t>& index = {}, bool amount64 = false, bool uncompressed = false) {
    const size_t pairs = keys.size() * ms.size();
    if (!index.empty() && index.size() != ms.size())
        throw std::logic_error("verify_find_tagged_serialized_mixed_keys: one index per proof");
    if (amounts.size() != (sealed ? ms.size() : pairs))
        throw std::logic_error("verify_find_tagged_serialized_mixed_keys: one sealed amount per proof, or K x count amounts");
    if (tags.size() != ms.size()) throw std::logic_error("verify_find_tagged_serialized_mixed_keys: one tag per proof");
    const size_t cap = std::min(max_hits, pairs);
    FindTaggedResult r;
    r.ok.assign(ms.size() + 1, 0);
    std::vector<uint32_t> rec(cap * 12 + 1);
    std::vector<uint8_t> packed(keys.size() * 32 + 1);
    for (size_t j = 0; j < keys.size(); j++)
        for (size_t t = 0; t < 32; t++) packed[j * 32 + t] = keys[j][t];
    const int flags = BPP_SER_TRANSCRIPT | (uncompressed ? BPP_SER_UNCOMPRESSED : 0) | (amount64 ? BPP_PROVE_AMOUNT64 : 0) |
                      (sealed ? BPP_FIND_AMOUNTS_SEALED : 0);
    uint32_t found = 0, candidates = 0;
    const int rc = bpp_range_verify_find_tagged_serialized_mixed_keys(
        engine, proofs.data(), commitments.data(), ms.data(), ms.size(), flags, packed.data(), keys.size(), index_base,
        index.empty() ? nullptr : index.data(), amounts.data(), r.ok.data(), rec.data(), cap, &found, tags.data(), &candidates);
    for (volatile uint8_t& b : packed) b = 0;   // the packed copy of the keys made here
    if (rc != BPP_OK)
        throw std::runtime_error(std::string("bpp_range_verify_find_tagged_serialized_mixed_keys: ") + bpp_last_error());
    r.ok.resize(ms.size());
    r.found = found;
    r.candidates = candidates;
    r.hits.resize(std::min<size_t>(found, cap));
    for (size_t h = 0; h < r.hits.size(); h++) {
        const uint32_t* w = rec.data() + h * 12;
        r.hits[h].key_no = w[0];
        r.hits[h].position = w[1];
        r.hits[h].amount = (uint64_t)w[2] | (uint64_t)w[3] << 32;
        for (int t = 0; t < 4; t++) r.hits[h].mask.e[t] = (uint64_t)w[4 + 2 * t] | (uint64_t)w[5 + 2 * t] << 32;
    }
    return r;
}

// The sender's side of outputs with derived masks (bpp_outputs_make): one recipient key, one amount per OUTPUT, ms[i] outputs
// in proof i, whose blinding index is index[i] or index_base + i.  masks: 4 words per output, the gamma layout of the commit
// and prove calls.  The masks are secret.
struct MadeOutputs {
    std::vector<uint64_t> masks, sealed;
    std::vector<uint8_t> tags;
};
inline MadeOutputs make_outputs(bpp_ctx* ctx, const std::vector<std::array<uint8_t, 32>>& keys, const std::vector<uint64_t>& amounts,
                                const std::vector<uint32_t>& ms, uint64_t index_base = 0, const std::vector<uint64_t>& index = {}) {
    size_t n_out = 0;
    for (uint32_t m : ms) n_out += m;
    if (keys.size() != n_out || amounts.size() != n_out) throw std::logic_error("make_outputs: one key and one amount per output");
    if (!index.empty() && index.size() != ms.size()) throw std::logic_error("make_outputs: one index per proof");
    std::vector<uint64_t> idx(n_out + 1);
    std::vector<uint32_t> place(n_out + 1);
    std::vector<uint8_t> packed(n_out * 32 + 1);
    for (size_t i = 0, o = 0; i < ms.size(); i++)
        for (uint32_t j = 0; j < ms[i]; j++, o++) {
            idx[o] = index.empty() ? index_base + i : index[i];
            place[o] = j;
            for (size_t t = 0; t < 32; t++) packed[o * 32 + t] = keys[o][t];
        }
    MadeOutputs r;
    r.masks.assign(n_out * 4 + 1, 0);
    r.sealed.assign(n_out + 1, 0);
    r.tags.assign(n_out + 1, 0);
    const int rc = bpp_outputs_make(ctx, packed.data(), idx.data(), place.data(), amounts.data(), n_out, r.masks.data(),
                                    r.sealed.data(), r.tags.data());
    for (volatile uint8_t& b : packed) b = 0;   // the packed copy of the keys made here
    if (rc != BPP_OK) throw std::runtime_error(std::string("bpp_outputs_make: ") + bpp_last_error());
    r.masks.resize(n_out * 4);
    r.sealed.resize(n_out);
    r.tags.resize(n_out);
    return r;
}

// Verifies a block and lists, per OUTPUT, what belongs to the keys, aggregated proofs included
// (bpp_range_verify_find_outputs_serialized_mixed_keys): sealed and tags hold one entry per output (sum of ms), in caller
// order, shared by all keys.  A hit's `position` is its output number.
inline FindTaggedResult verify_find_outputs_serialized_mixed_keys(
    bpp_verifier* engine, const std::vector<uint8_t>& proofs, const std::vector<uint8_t>& commitments,
    const std::vector<uint32_t>& ms, const std::vector<std::array<uint8_t, 32>>& keys, const std::vector<uint64_t>& sealed,
    const std::vector<uint8_t>& tags, size_t max_hits, uint64_t index_base = 0, const std::vector<uint64_t>& index = {},
    bool amount64 = false, bool uncompressed = false) {
    size_t n_out = 0;
    for (uint32_t m : ms) n_out += m;
    const size_t pairs = keys.size() * n_out;
    if (!index.empty() && index.size() != ms.size())
        throw std::logic_error("verify_find_outputs_serialized_mixed_keys: one index per proof");
    if (sealed.size() != n_out || tags.size() != n_out)
        throw std::logic_error("verify_find_outputs_serialized_mixed_keys: one sealed amount and one tag per output");
    const size_t cap = std::min(max_hits, pairs);
    FindTaggedResult r;
    r.ok.assign(ms.size() + 1, 0);
    std::vector<uint32_t> rec(cap * 12 + 1);
    std::vector<uint8_t> packed(keys.size() * 32 + 1);
    for (size_t j = 0; j < keys.size(); j++)
        for (size_t t = 0; t < 32; t++) packed[j * 32 + t] = keys[j][t];
    const int flags = BPP_SER_TRANSCRIPT | (uncompressed ? BPP_SER_UNCOMPRESSED : 0) | (amount64 ? BPP_PROVE_AMOUNT64 : 0);
    uint32_t found = 0, candidates = 0;
    const int rc = bpp_range_verify_find_outputs_serialized_mixed_keys(
        engine, proofs.data(), commitments.data(), ms.data(), ms.size(), flags, packed.data(), keys.size(), index_base,
        index.empty() ? nullptr : index.data(), sealed.data(), tags.data(), r.ok.data(), rec.data(), cap, &found, &candidates);
    for (volatile uint8_t& b : packed) b = 0;   // the packed copy of the keys made here
    if (rc != BPP_OK)
        throw std::runtime_error(std::string("bpp_range_verify_find_outputs_serialized_mixed_keys: ") + bpp_last_error());
    r.ok.resize(ms.size());
    r.found = found;
    r.candidates = candidates;
    r.hits.resize(std::min<size_t>(found, cap));
    for (size_t h = 0; h < r.hits.size(); h++) {
        const uint32_t* w = rec.data() + h * 12;
        r.hits[h].key_no = w[0];
        r.hits[h].position = w[1];
        r.hits[h].amount = (uint64_t)w[2] | (uint64_t)w[3] << 32;
        for (int t = 0; t < 4; t++) r.hits[h].mask.e[t] = (uint64_t)w[4 + 2 * t] | (uint64_t)w[5 + 2 * t] << 32;
    }
    return r;
}

// ---- proofs over ANY number of outputs (bpp_amd.h: the section of that name).  outs[i] in [1, m]: proof i is the proof of
// shape (n, 2^ceil(log2 outs[i])) over its values and masks padded with zeros; the streams carry the real outputs alone.
// The aggregation sizes of such a block, for an engine of capacity m (bpp_outs_shapes)
inline std::vector<uint32_t> outs_shapes(const std::vector<uint32_t>& outs, size_t m) {
    std::vector<uint32_t> ms(outs.size() + 1);
    if (bpp_outs_shapes(outs.data(), outs.size(), m, ms.data()) != BPP_OK)
        throw std::runtime_error(std::string("bpp_outs_shapes: ") + bpp_last_error());
    ms.resize(outs.size());
    return ms;
}

// Proves a ragged block (bpp_range_prove_batch_serialized_outs): values and gammas hold sum(outs) entries (gammas: 4 words
// each).  proof_bytes, point_bytes: of the whole container stream and of one encoded point, as the caller frames them
// (bpp_proof_bytes_version over outs_shapes; bpp_point_compressed_bytes / _uncompressed_bytes).
struct ProvedOutputs {
    std::vector<uint8_t> proofs, commitments;
};
inline ProvedOutputs prove_serialized_outputs(bpp_verifier* engine, const std::vector<uint64_t>& values,
                                              const std::vector<uint64_t>& gammas, const std::vector<uint32_t>& outs,
                                              size_t proof_bytes, size_t point_bytes, int flags = 0,
                                              const uint8_t* blind_key = nullptr, uint64_t index_base = 0) {
    size_t n_out = 0;
    for (uint32_t o : outs) n_out += o;
    if (values.size() != n_out || gammas.size() != n_out * 4)
        throw std::logic_error("prove_serialized_outputs: one value and one gamma per output");
    ProvedOutputs r;
    r.proofs.assign(proof_bytes + 1, 0);
    r.commitments.assign(n_out * point_bytes + 1, 0);
    if (bpp_range_prove_batch_serialized_outs(engine, values.data(), gammas.data(), outs.data(), outs.size(), flags, blind_key,
                                              index_base, r.proofs.data(), r.commitments.data()) != BPP_OK)
        throw std::runtime_error(std::string("bpp_range_prove_batch_serialized_outs: ") + bpp_last_error());
    r.proofs.resize(proof_bytes);
    r.commitments.resize(n_out * point_bytes);
    return r;
}

// Verifies a ragged block (bpp_range_verify_batch_serialized_outs): outs[i] encoded commitments per proof -> one status per
// proof, 0 Ok / 1 VerificationError / 2 FormatError
inline std::vector<uint32_t> verify_serialized_outputs(bpp_verifier* engine, const std::vector<uint8_t>& proofs,
                                                       const std::vector<uint8_t>& commitments, const std::vector<uint32_t>& outs,
                                                       int flags = 0) {
    std::vector<uint32_t> ok(outs.size() + 1);
    if (bpp_range_verify_batch_serialized_outs(engine, proofs.data(), commitments.data(), outs.data(), outs.size(), flags,
                                               ok.data()) != BPP_OK)
        throw std::runtime_error(std::string("bpp_range_verify_batch_serialized_outs: ") + bpp_last_error());
    ok.resize(outs.size());
    return ok;
}

// verify_find_outputs_serialized_mixed_keys over a ragged block (bpp_range_verify_find_outputs_serialized_outs_keys): sealed
// and tags hold one entry per REAL output (sum of outs); a hit's `position` counts real outputs only
inline FindTaggedResult verify_find_outputs_serialized_outs_keys(
    bpp_verifier* engine, const std::vector<uint8_t>& proofs, const std::vector<uint8_t>& commitments,
    const std::vector<uint32_t>& outs, const std::vector<std::array<uint8_t, 32>>& keys, const std::vector<uint64_t>& sealed,
    const std::vector<uint8_t>& tags, size_t max_hits, uint64_t index_base = 0, const std::vector<uint64_t>& index = {},
    bool amount64 = false, bool uncompressed = false) {
    size_t n_out = 0;
    for (uint32_t o : outs) n_out += o;
    const size_t pairs = keys.size() * n_out;
    if (!index.empty() && index.size() != outs.size())
        throw std::logic_error("verify_find_outputs_serialized_outs_keys: one index per proof");
    if (sealed.size() != n_out || tags.size() != n_out)
        throw std::logic_error("verify_find_outputs_serialized_outs_keys: one sealed amount and one tag per output");
    const size_t cap = std::min(max_hits, pairs);
    FindTaggedResult r;
    r.ok.assign(outs.size() + 1, 0);
    std::vector<uint32_t> rec(cap * 12 + 1);
    std::vector<uint8_t> packed(keys.size() * 32 + 1);
    for (size_t j = 0; j < keys.size(); j++)
        for (size_t t = 0; t < 32; t++) packed[j * 32 + t] = keys[j][t];
    const int flags = BPP_SER_TRANSCRIPT | (uncompressed ? BPP_SER_UNCOMPRESSED : 0) | (amount64 ? BPP_PROVE_AMOUNT64 : 0);
    uint32_t found = 0, candidates = 0;
    const int rc = bpp_range_verify_find_outputs_serialized_outs_keys(
        engine, proofs.data(), commitments.data(), outs.data(), outs.size(), flags, packed.data(), keys.size(), index_base,
        index.empty() ? nullptr : index.data(), sealed.data(), tags.data(), r.ok.data(), rec.data(), cap, &found, &candidates);
    for (volatile uint8_t& b : packed) b = 0;   // the packed copy of the keys made here
    if (rc != BPP_OK)
        throw std::runtime_error(std::string("bpp_range_verify_find_outputs_serialized_outs_keys: ") + bpp_last_error());
    r.ok.resize(outs.size());
    r.found = found;
    r.candidates = candidates;
    r.hits.resize(std::min<size_t>(found, cap));
    for (size_t h = 0; h < r.hits.size(); h++) {
        const uint32_t* w = rec.data() + h * 12;
        r.hits[h].key_no = w[0];
        r.hits[h].position = w[1];
        r.hits[h].amount = (uint64_t)w[2] | (uint64_t)w[3] << 32;
        for (int t = 0; t < 4; t++) r.hits[h].mask.e[t] = (uint64_t)w[4 + 2 * t] | (uint64_t)w[5 + 2 * t] << 32;
    }
    return r;
}

// Verifier-side holder of the commitments.  It exists only in the reference's (stale) README
// (README.md:47-55: RangeVerifier::new(), allocate(&prover.commitment_vec), proof.verify(.., &verifier));
// the reference's code takes the commitment slice directly (range/mod.rs:57-62).  Both forms are offered.
struct RangeVerifier {
    std::vector<Point> commitment_vec;
    void allocate(const std::vector<Point>& commitments) { commitment_vec = commitments; }
};

// WeightedInnerProductProof with prove (weighted_inner_product_proof.rs:36-227) and verify (:238-328) on the engine's WIP
// seam (bpp_amd.h, bpp_wip_prove_batch / bpp_wip_verify_batch).  power_of_y_vec must be [y, y^2, .., y^len]: as the
// reference's verify (:252, :276) only its first entry is read, the engine rebuilds the rest.  engine: an engine created
// for this key (bpp_verifier_create, n m = len); null: a small one (window_bits 4) is created for the call.
struct WeightedInnerProductProof {
    std::vector<Point> L_vec, R_vec;
    Point A, B;
    PrimeFieldElem r_prime, s_prime, d_prime;

    // `commitment` is dead in the reference (:57, :137-142) and is ignored
    static WeightedInnerProductProof prove(const PublicKey& pk, const std::vector<PrimeFieldElem>& a_vec,
                                           const std::vector<PrimeFieldElem>& b_vec,
                                           const std::vector<PrimeFieldElem>& power_of_y_vec, const PrimeFieldElem& gamma,
                                           const Point& commitment, bpp_verifier* engine = nullptr) {
        (void)commitment;
        const size_t len = pk.G_vec.size(), pw = Arith::point_words();
        if (pk.H_vec.size() != len || a_vec.size() != len || b_vec.size() != len || power_of_y_vec.size() != len ||
            len == 0 || (len & (len - 1)))
            throw std::logic_error("assertion failed: vectors of one power-of-two length");              // :60-67
        size_t k = 0;
        while (((size_t)1 << k) < len) k++;
        Engine eng(pk, engine);
        std::vector<uint64_t> a = flat(a_vec), b = flat(b_vec), pts((3 + 2 * k) * pw), sc(12);
        if (bpp_wip_prove_batch(eng.e, a.data(), b.data(), power_of_y_vec[0].e.data(), gamma.e.data(), 1, 0, 0, nullptr,
                                nullptr, 0, nullptr, pts.data(), sc.data(), nullptr) != BPP_OK)
            throw std::runtime_error(std::string("bpp_wip_prove_batch: ") + bpp_last_error());
        WeightedInnerProductProof p;
        p.A = Point(pts.data() + pw);
        p.B = Point(pts.data() + 2 * pw);
        for (size_t i = 0; i < k; i++) {
            p.L_vec.emplace_back(pts.data() + (3 + i) * pw);
            p.R_vec.emplace_back(pts.data() + (3 + k + i) * pw);
        }
        p.r_prime = PrimeFieldElem::from_limbs(sc.data());
        p.s_prime = PrimeFieldElem::from_limbs(sc.data() + 4);
        p.d_prime = PrimeFieldElem::from_limbs(sc.data() + 8);
        return p;
    }

    // Ok(()) -> std::nullopt ; Err(ProofError::VerificationError) -> the error; the four *_exp arguments are the
    // *_exp_of_commitment of :238-247
    std::optional<ProofError> verify(const PublicKey& pk, const std::vector<PrimeFieldElem>& power_of_y_vec,
                                     const std::vector<PrimeFieldElem>& G_exp, const std::vector<PrimeFieldElem>& H_exp,
                                     const PrimeFieldElem& g_exp, const std::vector<PrimeFieldElem>& V_exp,
                                     const Point& A_prime, const std::vector<Point>& V, bpp_verifier* engine = nullptr) const {
        const size_t len = pk.G_vec.size(), k = L_vec.size();
        if (len != ((size_t)1 << k) || R_vec.size() != k) return ProofError::VerificationError;            // :335-337
        if (G_exp.size() != len || H_exp.size() != len || V_exp.size() != V.size() || power_of_y_vec.size() != len)
            throw std::logic_error("mulvec: lengths of scalars and points must match");                    // mulvec.rs:23-25
        Engine eng(pk, engine);
        std::vector<uint64_t> pts(A_prime.w);
        pts.insert(pts.end(), A.w.begin(), A.w.end());
        pts.insert(pts.end(), B.w.begin(), B.w.end());
        for (auto& p : L_vec) pts.insert(pts.end(), p.w.begin(), p.w.end());
        for (auto& p : R_vec) pts.insert(pts.end(), p.w.begin(), p.w.end());
        for (auto& p : V) pts.insert(pts.end(), p.w.begin(), p.w.end());
        std::vector<uint64_t> stm = flat(G_exp), h = flat(H_exp), vc = flat(V_exp);
        stm.insert(stm.end(), h.begin(), h.end());
        stm.insert(stm.end(), g_exp.e.begin(), g_exp.e.end());
        stm.insert(stm.end(), vc.begin(), vc.end());
        uint64_t sc[12];
        std::memcpy(sc, r_prime.e.data(), 32);
        std::memcpy(sc + 4, s_prime.e.data(), 32);
        std::memcpy(sc + 8, d_prime.e.data(), 32);
        uint32_t ok = 1;
        if (bpp_wip_verify_batch(eng.e, pts.data(), sc, power_of_y_vec[0].e.data(), stm.data(), V.size(), 1, 0, nullptr,
                                 nullptr, &ok, nullptr, nullptr) != BPP_OK)
            throw std::runtime_error(std::string("bpp_wip_verify_batch: ") + bpp_last_error());
        if (ok == 0) return std::nullopt;
        return ProofError::VerificationError;
    }

  private:
    static std::vector<uint64_t> flat(const std::vector<PrimeFieldElem>& v) {
        std::vector<uint64_t> o;
        for (auto& x : v) o.insert(o.end(), x.e.begin(), x.e.end());
        return o;
    }
    // the caller's engine, or one of its own for the length of the key (only n m = len counts; n <= 64)
    struct Engine {
        bpp_verifier* e;
        bool own;
        Engine(const PublicKey& pk, bpp_verifier* given) : e(given), own(false) {
            if (e) return;
            const size_t len = pk.G_vec.size(), n = len < 64 ? len : 64;
            auto gh = pk.gh_wire(), G = PublicKey::flat(pk.G_vec), H = PublicKey::flat(pk.H_vec);
            if (bpp_verifier_create(Arith::ctx(), gh.data(), G.data(), H.data(), n, len / n, 4, &e) != BPP_OK)
                throw std::runtime_error(std::string("bpp_verifier_create: ") + bpp_last_error());
            own = true;
        }
        Engine(const Engine&) = delete;
        Engine& operator=(const Engine&) = delete;
        ~Engine() {
            if (own) bpp_verifier_destroy(e);
        }
    };
};

struct RangeProof {
    Point A;
    WeightedInnerProductProof proof;

    static RangeProof prove(const PublicKey& pk, size_t n, const RangeProver& prover) {   // range/mod.rs:31-55
        const size_t m = prover.v_vec.size(), mn = n * m, pw = Arith::point_words();
        if (m == 0 || (mn & (mn - 1))) throw std::logic_error("n * m must be a power of two");        // wip.rs:67
        if (pk.G_vec.size() != mn || pk.H_vec.size() != mn)
            throw std::logic_error("assertion failed: pk.G_vec.len() == n * m");                       // range/mod.rs:90-91,252-253
        size_t k = 0;
        while (((size_t)1 << k) < mn) k++;
        auto gh = pk.gh_wire(), G = PublicKey::flat(pk.G_vec), H = PublicKey::flat(pk.H_vec);
        auto V = PublicKey::flat(prover.commitment_vec);
        std::vector<uint64_t> gm;
        for (auto& g : prover.gamma_vec) gm.insert(gm.end(), g.e.begin(), g.e.end());
        std::vector<uint64_t> pts((3 + 2 * k) * pw), sc(12);
        if (bpp_range_prove(Arith::ctx(), gh.data(), G.data(), H.data(), n, m, prover.v_vec.data(), gm.data(), V.data(),
                            pts.data(), sc.data()) != BPP_OK)
            throw std::runtime_error(std::string("bpp_range_prove: ") + bpp_last_error());
        RangeProof rp;
        rp.A = Point(pts.data());
        rp.proof.A = Point(pts.data() + pw);
        rp.proof.B = Point(pts.data() + 2 * pw);
        for (size_t i = 0; i < k; i++) {
            rp.proof.L_vec.emplace_back(pts.data() + (3 + i) * pw);
            rp.proof.R_vec.emplace_back(pts.data() + (3 + k + i) * pw);
        }
        rp.proof.r_prime = PrimeFieldElem::from_limbs(sc.data());
        rp.proof.s_prime = PrimeFieldElem::from_limbs(sc.data() + 4);
        rp.proof.d_prime = PrimeFieldElem::from_limbs(sc.data() + 8);
        return rp;
    }

    // Ok(()) -> std::nullopt ; Err(ProofError::VerificationError) -> the error   (range/mod.rs:57-78)
    std::optional<ProofError> verify(const PublicKey& pk, size_t n, const std::vector<Point>& commitment_vec) const {
        const size_t m = commitment_vec.size(), k = proof.L_vec.size();
        auto gh = pk.gh_wire(), G = PublicKey::flat(pk.G_vec), H = PublicKey::flat(pk.H_vec);
        auto V = PublicKey::flat(commitment_vec);
        std::vector<uint64_t> pts(A.w);
        pts.insert(pts.end(), proof.A.w.begin(), proof.A.w.end());
        pts.insert(pts.end(), proof.B.w.begin(), proof.B.w.end());
        for (auto& p : proof.L_vec) pts.insert(pts.end(), p.w.begin(), p.w.end());
        for (auto& p : proof.R_vec) pts.insert(pts.end(), p.w.begin(), p.w.end());
        uint64_t sc[12];
        std::memcpy(sc, proof.r_prime.e.data(), 32);
        std::memcpy(sc + 4, proof.s_prime.e.data(), 32);
        std::memcpy(sc + 8, proof.d_prime.e.data(), 32);
        int rc = bpp_range_verify(Arith::ctx(), gh.data(), G.data(), H.data(), n, m, pts.data(), k, sc, V.data());
        if (rc == BPP_OK) return std::nullopt;
        if (rc == BPP_VERIFICATION_ERROR) return ProofError::VerificationError;
        throw std::runtime_error(std::string("bpp_range_verify: ") + bpp_last_error());
    }
    std::optional<ProofError> verify(const PublicKey& pk, size_t n, const RangeVerifier& verifier) const {
        return verify(pk, n, verifier.commitment_vec);
    }
};

// RangeProof::prove (range/mod.rs:31-55) for a block in which proof i has values[i].size() = m_i values (a power of two <= the
// engine's m), each against the prefix key PublicKey::new(n m_i) (bpp_range_prove_batch_mixed, literal challenges and
// blinding): each proof with its commitments.  amount64 = false: RangeProver::commit's commitments, with the `v as i32` of
// range/prover.rs:37; true (BPP_PROVE_AMOUNT64): V = v g + gamma h over the whole u64, so an amount of 2^31 or more proves
// and verifies.  n: the engine's bits per value.
inline std::vector<std::pair<RangeProof, std::vector<Point>>> prove_batch_mixed(
    bpp_verifier* engine, size_t n, const std::vector<std::vector<uint64_t>>& values,
    const std::vector<std::vector<PrimeFieldElem>>& gammas, bool amount64 = false) {
    if (values.size() != gammas.size()) throw std::logic_error("prove_batch_mixed: one gamma list per proof");
    const size_t pw = Arith::point_words();
    auto log2of = [](size_t x) {
        size_t k = 0;
        while (((size_t)1 << k) < x) k++;
        return k;
    };
    std::vector<uint64_t> vs, gw;
    std::vector<uint32_t> ms;
    size_t npts = 0;
    for (size_t i = 0; i < values.size(); i++) {
        if (values[i].size() != gammas[i].size()) throw std::logic_error("prove_batch_mixed: one gamma per value");
        vs.insert(vs.end(), values[i].begin(), values[i].end());
        for (auto& g : gammas[i]) gw.insert(gw.end(), g.e.begin(), g.e.end());
        ms.push_back((uint32_t)values[i].size());
        npts += 3 + 2 * log2of(n * values[i].size()) + values[i].size();
    }
    std::vector<uint64_t> pts(npts * pw + 1), sc(values.size() * 12 + 1);
    if (bpp_range_prove_batch_mixed(engine, vs.data(), gw.data(), ms.data(), values.size(), amount64 ? BPP_PROVE_AMOUNT64 : 0,
                                    nullptr, 0, pts.data(), sc.data(), nullptr) != BPP_OK)
        throw std::runtime_error(std::string("bpp_range_prove_batch_mixed: ") + bpp_last_error());
    std::vector<std::pair<RangeProof, std::vector<Point>>> out;
    size_t at = 0;
    for (size_t i = 0; i < values.size(); i++) {
        const size_t k = log2of(n * values[i].size());
        const uint64_t* p = pts.data() + at * pw;
        RangeProof rp;
        rp.A = Point(p);
        rp.proof.A = Point(p + pw);
        rp.proof.B = Point(p + 2 * pw);
        for (size_t t = 0; t < k; t++) {
            rp.proof.L_vec.emplace_back(p + (3 + t) * pw);
            rp.proof.R_vec.emplace_back(p + (3 + k + t) * pw);
        }
        rp.proof.r_prime = PrimeFieldElem::from_limbs(sc.data() + 12 * i);
        rp.proof.s_prime = PrimeFieldElem::from_limbs(sc.data() + 12 * i + 4);
        rp.proof.d_prime = PrimeFieldElem::from_limbs(sc.data() + 12 * i + 8);
        std::vector<Point> V;
        for (size_t j = 0; j < values[i].size(); j++) V.emplace_back(p + (3 + 2 * k + j) * pw);
        out.emplace_back(std::move(rp), std::move(V));
        at += 3 + 2 * k + values[i].size();
    }
    return out;
}

}  // namespace bpp
