// impl_wip.hpp -- host side of the WIP seam (wip_seam.hpp): bpp_wip_prove_batch_device / bpp_wip_verify_batch_device and
// their host-buffer forms, on an engine's tables.  One instantiation per curve (tu_wip_*.hip).
//
// The verifier is VerifyImpl::run_stage -- the pass prologue, layout carver, proof-point MSM, fixed-generator MulVec and
// verdicts of bpp_verifier_run -- with the seam's two scalar kernels as its scalar stage and a pass shape of its own
// (wip_verify_shape).  The prover is k_wip_px, the blinding, k_wip_init (k_wip_fs_start) and k_wip_challenges_out around
// ProveBatchImpl::argument (impl_prove_batch.hpp), the schedule it shares with the range prover: the kernels of
// prover_batch.hpp are launched from there, this unit compiles k_wip_* and k_wvs_* alone.
#pragma once
#include "impl_prove_batch.hpp"
#include "wip_seam.hpp"

namespace bpp {

constexpr uint32_t WIP_E_ROUND = 7, WIP_E_FINAL = 99;   // wip.rs:131 / :353, :211 / :369

// What a seam prove call takes, in the C ABI's order; the device's pointers for prove_device, the host's for prove_host
// (blind_key, 32 bytes: the host's always).  a, b: count x len scalars ; y, gamma: count scalars ; transcript: count x 32
// bytes of state, read when fs ; blinding: count x (5 + 2k) canonical scalars, or blind_key with proof i's index
// index_base + i, or the literals.  points: count records of 3 + 2k + nv wire points, point 0 and the last nv of each the
// caller's, the rest written ; out_scalars: count x 3 ; out_challenges (may be null): count x (1 + k), [e, e_1..e_k].
struct WipProveArgs {
    const uint64_t *a = nullptr, *b = nullptr, *y = nullptr, *gamma = nullptr;
    size_t count = 0, nv = 0;
    bool fs = false;
    const void* transcript = nullptr;
    const uint8_t* blind_key = nullptr;
    uint64_t index_base = 0;
    const uint64_t* blinding = nullptr;
    uint64_t *points = nullptr, *out_scalars = nullptr, *out_challenges = nullptr;
};

template <class C>
struct WipImpl {
    using V = VerifyImpl<C>;
    using PB = ProveBatchImpl<C>;
    static constexpr int WW = V::WW;
    static constexpr int JW = V::JW;

    // The pass shape of the seam's verifier on engine v: mn = len, m = nv statement points, NV = 3 + 2k + nv,
    // N = 2 len + 2k + 5 + nv, head in the order of wip.rs:309-311.  It drives k_fixed_msm, k_var_* and k_finalize* as the
    // engine's own shape does (same tables, same generators).
    static VerifyShape verify_shape(const bpp_verifier* v, size_t nv) {
        VerifyShape s = v->s;
        s.m = (uint32_t)nv;
        s.NV = 3 + 2 * s.k + (uint32_t)nv;
        s.N = 2 * s.mn + 2 * s.k + 5 + (uint32_t)nv;
        s.head_wip = 1;
        return s;
    }
    // ... and of its prover: no commitments, so 2k + 3 virtual-proof slots of 2 len + 2k + 5 scalars (slot 0 unused)
    static VerifyShape prove_shape(const bpp_verifier* v) { return verify_shape(v, 0); }

    // ---- prover: workspace = the range prover's layout for the seam's shape | the chunk's px entries -----------------
    struct ProveWs {
        typename PB::ProveLayout run;
        size_t px, total;
    };
    static ProveWs prove_ws(const bpp_verifier* v, size_t count) {
        ProveWs w;
        w.run = PB::prove_layout(prove_shape(v), count);
        WsCarver o;
        o.take(w.run.total);
        w.px = o.take(w.run.chunk * (size_t)PX_WORDS * 4);
        w.total = o.total;
        return w;
    }
    static int prove_device(bpp_verifier* v, const WipProveArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);
    static int prove_host(bpp_verifier* v, const WipProveArgs& a);

    // ---- verifier: workspace = challenges derived from the transcript | the pass's workspace (ws_layout) ---------------
    struct VerifyWs {
        size_t ch, run, total;
    };
    static VerifyWs verify_ws(const bpp_verifier* v, size_t count, size_t nv) {
        const VerifyShape s = verify_shape(v, nv);
        VerifyWs w;
        WsCarver o;
        w.ch = o.take(count * (size_t)(1 + s.k) * 32);
        w.run = o.take(V::ws_layout(s, count).total);
        w.total = o.total;
        return w;
    }
    static int verify_device(bpp_verifier* v, const uint64_t* d_points, const uint64_t* d_scalars, const uint64_t* d_y,
                             const uint64_t* d_statement, size_t nv, size_t count, bool fs, const void* d_transcript,
                             const uint64_t* d_challenges, uint32_t* d_ok, void* d_workspace, size_t workspace_bytes,
                             uint64_t* d_out_scalars, uint64_t* d_out_result, hipStream_t st);
    static int verify_host(bpp_verifier* v, const uint64_t* points, const uint64_t* scalars, const uint64_t* y,
                           const uint64_t* statement, size_t nv, size_t count, bool fs, const void* transcript,
                           const uint64_t* challenges, uint32_t* out_ok, uint64_t* out_scalars, uint64_t* out_result);
};

#ifdef BPP_IMPL_DEFINITIONS
template <class C>
int WipImpl<C>::prove_device(bpp_verifier* v, const WipProveArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
    const VerifyShape s = prove_shape(v);
    const uint32_t k = s.k;
    const uint32_t nvp = pb_num_vps(k, s.m);            // 2k + 3
    const uint32_t rec_stride = 3 + 2 * k + (uint32_t)a.nv;
    if ((a.count * rec_stride) >> 32) return fail(BPP_E_ARG, "count too large");
    const ProveWs Lw = prove_ws(v, a.count);
    if (workspace_bytes < Lw.total) return fail(BPP_E_ARG, "workspace too small");
    const typename PB::ProveLayout& L = Lw.run;
    const ProverConsts pc = PB::literals();   // alpha and amount64 are the range statement's: not read, no commitment formed
    const WipLiterals lit{WIP_E_ROUND, WIP_E_FINAL};
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    auto U32 = [](const uint64_t* q) { return reinterpret_cast<const uint32_t*>(q); };
    uint32_t* px = W(Lw.px);
    for (size_t base = 0; base < a.count; base += L.chunk) {
        const size_t cnt = std::min(L.chunk, a.count - base);
        hipLaunchKernelGGL(k_wip_px, dim3(cdiv(cnt, 256)), dim3(256), 0, st, px, base, rec_stride, cnt);
        // records and triples go through px, whose PX_CALLER carries base + p; the challenges are hashed into the workspace's
        // 3 + k blocks, the caller's are [e, e_1..e_k]
        typename PB::Chunk c{s, pc, L, ws, cnt, a.blinding ? U32(a.blinding) + base * (size_t)pb_blind_elems(k) * 8 : nullptr,
                             px, reinterpret_cast<uint32_t*>(a.points), nullptr, reinterpret_cast<uint32_t*>(a.out_scalars),
                             W(L.ch), st, v->table.u32()};
        PB::chunk_blinding(c, a.blind_key, a.index_base);
        hipLaunchKernelGGL(k_wip_init<C>, dim3((unsigned)cnt), dim3(256), 0, st, s, lit, a.fs ? 1u : 0u,
                           U32(a.a) + base * (size_t)s.mn * 8, U32(a.b) + base * (size_t)s.mn * 8, U32(a.y) + base * 8,
                           U32(a.gamma) + base * 8, W(L.a), W(L.b), W(L.cG), W(L.cH), W(L.pwy), W(L.con), W(L.vps));
        if (a.fs)
            hipLaunchKernelGGL(k_wip_fs_start<C>, dim3(cdiv(cnt, 64)), dim3(64), 0, st, s,
                               static_cast<const uint8_t*>(a.transcript) + base * 32, W(L.trst), cnt);
        PB::argument(c, a.fs, VpSel{nvp, 1u, 2 * k + 2, 1u});   // literal mode: L_t, R_t, wip.A, wip.B, the virtual proofs that exist
        if (a.out_challenges)
            hipLaunchKernelGGL(k_wip_challenges_out<C>, dim3((unsigned)cnt), dim3(64), 0, st, k, lit,
                               a.fs ? W(L.ch) : (const uint32_t*)nullptr,
                               reinterpret_cast<uint32_t*>(a.out_challenges) + base * (size_t)(1 + k) * 8);
    }
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int WipImpl<C>::verify_device(bpp_verifier* v, const uint64_t* d_points, const uint64_t* d_scalars, const uint64_t* d_y,
                              const uint64_t* d_statement, size_t nv, size_t count, bool fs, const void* d_transcript,
                              const uint64_t* d_challenges, uint32_t* d_ok, void* d_workspace, size_t workspace_bytes,
                              uint64_t* d_out_scalars, uint64_t* d_out_result, hipStream_t st) {
    const VerifyShape s = verify_shape(v, nv);
    const VerifyWs L = verify_ws(v, count, nv);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    if (wvs_lds_bytes<C>(s) > 64 * 1024) return fail(BPP_E_ARG, "n*m too large for the seam's scalar kernels");
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    const uint32_t* ch = reinterpret_cast<const uint32_t*>(d_challenges);   // the caller's own transcript comes first
    if (!ch && fs) {
        uint32_t* w_ch = reinterpret_cast<uint32_t*>(ws + L.ch);
        hipLaunchKernelGGL(k_wip_transcript_challenges<C>, dim3(cdiv(count, 64)), dim3(64), 0, st, s,
                           static_cast<const uint8_t*>(d_transcript), reinterpret_cast<const uint32_t*>(d_points), w_ch, count);
        ch = w_ch;
    }
    const WipLiterals lit{WIP_E_ROUND, WIP_E_FINAL};
    return V::run_stage(
        v, s, d_points, count,
        [&](uint32_t* w_sc, uint32_t* w_prep, uint32_t* w_bad, hipStream_t st_) -> int {
            hipLaunchKernelGGL(k_wvs_prepare<C>, dim3(cdiv(count, 64)), dim3(64), 0, st_, s, lit,
                               reinterpret_cast<const uint32_t*>(d_scalars), reinterpret_cast<const uint32_t*>(d_y),
                               reinterpret_cast<const uint32_t*>(d_statement), ch, w_prep, w_sc, w_bad, count);
            hipLaunchKernelGGL(k_wvs_expand<C>, dim3(cdiv(count, VS_PB)), dim3(VS_BLOCK), wvs_lds_bytes<C>(s), st_, s, w_prep,
                               reinterpret_cast<const uint32_t*>(d_statement), w_sc, count);
            HIPCHK(hipGetLastError());
            return BPP_OK;
        },
        d_ok, ws + L.run, workspace_bytes - L.run, d_out_scalars, d_out_result, st);
}

// The two host forms stage through DevBuf (staging.hpp): blocking copies, where they used to enqueue asynchronous ones on
// the null stream and synchronise -- from and to pageable host memory that is the same transfer, and the device entries'
// launches on the null stream are ordered between the copies as before.  A failed entry returns at once: the buffers'
// hipFree waits for whatever was enqueued.
template <class C>
int WipImpl<C>::prove_host(bpp_verifier* v, const WipProveArgs& a) {
    const VerifyShape s = prove_shape(v);
    const uint32_t k = s.k;
    const size_t count = a.count;
    const size_t pts_bytes = count * (size_t)(3 + 2 * k + a.nv) * WW * 4, ch_bytes = count * (size_t)(1 + k) * 32;
    DevBuf da, db, dy, dg, dtr, dbl, dpts, dsc, dch, dws;
    HIPCHK(da.upload(a.a, count * (size_t)s.mn * 32));
    HIPCHK(db.upload(a.b, count * (size_t)s.mn * 32));
    HIPCHK(dy.upload(a.y, count * 32));
    HIPCHK(dg.upload(a.gamma, count * 32));
    HIPCHK(dtr.upload(a.fs ? a.transcript : nullptr, count * 32));
    HIPCHK(dbl.upload(a.blinding, count * (size_t)pb_blind_elems(k) * 32));
    HIPCHK(dpts.upload(a.points, pts_bytes));   // point 0 and the last nv of a record are the caller's
    HIPCHK(dsc.alloc(count * 96));
    if (a.out_challenges) HIPCHK(dch.alloc(ch_bytes));
    const size_t wsb = prove_ws(v, count).total;
    HIPCHK(dws.alloc(wsb));
    const WipProveArgs d{da.u64(), db.u64(),    dy.u64(),     dg.u64(),  count,      a.nv,      a.fs,   // the record's order
                         dtr.p,    a.blind_key, a.index_base, dbl.u64(), dpts.u64(), dsc.u64(), dch.u64()};
    BPP_TRY(prove_device(v, d, dws.p, wsb, nullptr));
    HIPCHK(dpts.download(a.points, pts_bytes));
    HIPCHK(dsc.download(a.out_scalars, count * 96));
    if (a.out_challenges) HIPCHK(dch.download(a.out_challenges, ch_bytes));
    return BPP_OK;
}

template <class C>
int WipImpl<C>::verify_host(bpp_verifier* v, const uint64_t* points, const uint64_t* scalars, const uint64_t* y,
                            const uint64_t* statement, size_t nv, size_t count, bool fs, const void* transcript,
                            const uint64_t* challenges, uint32_t* out_ok, uint64_t* out_scalars, uint64_t* out_result) {
    const VerifyShape s = verify_shape(v, nv);
    DevBuf dp, dsc, dy, dstm, dtr, dch, dok, dos, dres, dws;
    HIPCHK(dp.upload(points, count * (size_t)s.NV * WW * 4));
    HIPCHK(dsc.upload(scalars, count * 96));
    HIPCHK(dy.upload(y, count * 32));
    HIPCHK(dstm.upload(statement, count * (size_t)wip_statement_elems(s) * 32));
    HIPCHK(dtr.upload(transcript, count * 32));
    HIPCHK(dch.upload(challenges, count * (size_t)(1 + s.k) * 32));
    HIPCHK(dok.alloc(count * 4));
    if (out_scalars) HIPCHK(dos.alloc(count * (size_t)s.N * 32));
    if (out_result) HIPCHK(dres.alloc(count * (size_t)WW * 4));
    const size_t wsb = verify_ws(v, count, nv).total;
    HIPCHK(dws.alloc(wsb));
    BPP_TRY(verify_device(v, dp.u64(), dsc.u64(), dy.u64(), dstm.u64(), nv, count, fs, dtr.p, dch.u64(), dok.u32(), dws.p, wsb,
                          dos.u64(), dres.u64(), nullptr));
    HIPCHK(dok.download(out_ok, count * 4));
    if (out_scalars) HIPCHK(dos.download(out_scalars, count * (size_t)s.N * 32));
    if (out_result) HIPCHK(dres.download(out_result, count * (size_t)WW * 4));
    return BPP_OK;
}
#endif  // BPP_IMPL_DEFINITIONS

extern template struct WipImpl<Bls12381>;
extern template struct WipImpl<Secp256k1>;
extern template struct WipImpl<Ed25519>;

}  // namespace bpp
