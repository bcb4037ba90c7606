// commit.hpp -- bpp_commit_batch_device / bpp_commit_batch: RangeProver::commit (reference src/range/prover.rs:28-42) for a
// block of values over an engine's g and h.  One instantiation per curve (tu_commit_*.hip).
//
// Inside the prover a commitment is a virtual proof of k_fixed_msm with two terms: two lanes of one 128-thread block work
// and the block's partials go through the folds and k_pb_collect.  As a seam of its own it is one lane per commitment
// (k_commit_batch): the lane walks the window-table rows of generators 0 and 1 (commit_walk.hpp), one gather by ordinary
// vector loads and one lazy mixed addition per non-zero digit, converts its sum to the affine wire point itself (one
// fe_inv) and stores it.  No LDS, no workspace, no partials.  The lanes of a wave diverge only in WHICH digits are zero;
// a step no lane of the wave needs is skipped by the branch.
#pragma once
#include "impl_verify.hpp"

#include "commit_walk.hpp"

namespace bpp {

static_assert(commit_walk_glv<Bls12381>() == fixed_glv<Bls12381>() && commit_walk_glv<Secp256k1>() == fixed_glv<Secp256k1>() &&
                  commit_walk_glv<Ed25519>() == fixed_glv<Ed25519>(),
              "the walk reads the tables in the layout the verifier built them in");

constexpr unsigned COMMIT_BLOCK = 64;

// values: [count] u64 ; gammas: [count][8] scalars, read as k_pb_init reads them (through the field: reduced mod r) ;
// out_V: [count] wire points.  amount64 = 0: the scalar on g is new(v as i32) (prover.rs:37), else the whole u64.
template <class C>
__global__ void __launch_bounds__(COMMIT_BLOCK) k_commit_batch(VerifyShape s, const uint32_t* __restrict__ table,
                                                               const uint64_t* __restrict__ values,
                                                               const uint32_t* __restrict__ gammas, uint32_t amount64,
                                                               uint32_t* __restrict__ out_V, size_t count) {
    using P = typename C::Fr;
    constexpr int N = C::Fp::N;
    constexpr int WW = 2 * N + 2;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint32_t kv[8], kg[8];
    commit_amount_scalar<C>(values[i], amount64 != 0, kv);
    ld_words<8>(gammas + i * 8, kg);
    fe_to_canonical(fe_from_canonical<P>(kg), kg);
    const Xyzz<C> acc = commit_walk<C>(
        s, kv, kg, [&](size_t e) { return aff_ldg<C>(table + e * (size_t)(2 * N)); },
        [](Xyzz<C>& a, const Aff<C>& q, bool neg) { xyzz_madd_lazy(a, q, neg); });
    uint32_t w[WW];
    aff_to_wire(jac_to_aff(xyzz_to_jac(acc)), w);   // the conversion k_pb_collect applies to the prover's commitments
    uint32_t* dst = out_V + i * (size_t)WW;
#pragma unroll
    for (int t = 0; t < WW; t++) dst[t] = w[t];
}

template <class C>
struct CommitImpl {
    static constexpr int WW = 2 * C::Fp::N + 2;
    // enqueues on st; nothing else
    static int commit_batch_device(bpp_verifier* v, const uint64_t* d_values, const uint64_t* d_gammas, size_t count,
                                   bool amount64, uint64_t* d_out_V, hipStream_t st);
    // host buffers in, host buffers out
    static int commit_batch(bpp_verifier* v, const uint64_t* values, const uint64_t* gammas, size_t count, bool amount64,
                            uint64_t* out_V);
};

#ifdef BPP_IMPL_DEFINITIONS
template <class C>
int CommitImpl<C>::commit_batch_device(bpp_verifier* v, const uint64_t* d_values, const uint64_t* d_gammas, size_t count,
                                       bool amount64, uint64_t* d_out_V, hipStream_t st) {
    hipLaunchKernelGGL(k_commit_batch<C>, dim3(cdiv(count, COMMIT_BLOCK)), dim3(COMMIT_BLOCK), 0, st, v->s, v->table.u32(),
                       d_values, reinterpret_cast<const uint32_t*>(d_gammas), amount64 ? 1u : 0u,
                       reinterpret_cast<uint32_t*>(d_out_V), count);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int CommitImpl<C>::commit_batch(bpp_verifier* v, const uint64_t* values, const uint64_t* gammas, size_t count, bool amount64,
                                uint64_t* out_V) {
    // (blocking copies where asynchronous ones on the null stream and a synchronise stood: the same transfers)
    DevBuf d_val, d_gam, d_V;
    HIPCHK(d_val.upload(values, count * 8));
    BPP_TRY(upload_scalars<C>(gammas, count, d_gam, nullptr));
    HIPCHK(d_V.alloc(count * (size_t)WW * 4));
    BPP_TRY(commit_batch_device(v, d_val.u64(), d_gam.u64(), count, amount64, d_V.u64(), nullptr));
    HIPCHK(d_V.download(out_V, count * (size_t)WW * 4));
    return BPP_OK;
}
#endif  // BPP_IMPL_DEFINITIONS

extern template struct CommitImpl<Bls12381>;
extern template struct CommitImpl<Secp256k1>;
extern template struct CommitImpl<Ed25519>;

}  // namespace bpp
