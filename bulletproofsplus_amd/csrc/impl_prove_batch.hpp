// impl_prove_batch.hpp -- the engine's batched prover (bpp_range_prove_batch*, the mixed prove entries) on a verifier's
// window tables, and the ONE schedule of the weighted inner product argument (k rounds and the final step, the MulVecs and
// the hashing between them) that it shares with the WIP seam (impl_wip.hpp).  One instantiation per curve
// (tu_prove_*.hip): the kernels of prover_batch.hpp and k_fixed_msm<C, 2> are launched from those units alone.
#pragma once
#include "impl_verify.hpp"
#include "prover_batch.hpp"

namespace bpp {

template <class C>
struct ProveBatchImpl {
    using V = VerifyImpl<C>;
    static constexpr int JW = V::JW, WW = V::WW;

    // Device-resident form: values, gammas, outputs and workspace are device buffers, nothing touches the host
    // and nothing synchronises.  The batch is processed in chunks that reuse one workspace.
    struct ProveLayout {
        size_t a, b, cG, cH, pwy, con, vps, part, part1, part2, vout, trst, ch, blind, vals, gams, total;
        size_t chunk;
        unsigned per;
    };
    static size_t prove_chunk(const VerifyShape& s, size_t count) {
        const uint32_t nvp = pb_num_vps(s.k, s.m);
        const size_t chunk_max = std::max<size_t>(1, std::min<size_t>(2048, ((size_t)12 << 30) / ((size_t)nvp * s.N * 32)));
        return std::min(chunk_max, std::max<size_t>(count, 1));
    }
    // mixed: one class of a mixed block -- a chunk's values and gammas are gathered out of the caller's packed buffers
    static ProveLayout prove_layout(const VerifyShape& s, size_t count, bool mixed = false) {
        ProveLayout w;
        const uint32_t nvp = pb_num_vps(s.k, s.m);
        w.chunk = prove_chunk(s, count);
        const size_t nv_total = w.chunk * nvp;
        w.per = blocks_per_proof(s, nv_total);
        const size_t vec = w.chunk * (size_t)s.mn * 32;
        WsCarver o;
        w.a = o.take(vec);
        w.b = o.take(vec);
        w.cG = o.take(vec);
        w.cH = o.take(vec);
        w.pwy = o.take(vec);
        w.con = o.take(w.chunk * (size_t)pb_consts_elems(s.k) * 32);
        w.vps = o.take(nv_total * (size_t)s.N * 32);
        w.part = o.take(nv_total * w.per * FIXED_BLOCK * JW * 4);                                // one partial per thread
        w.part1 = o.take(nv_total * w.per * (FIXED_BLOCK / FOLD_GROUP) * JW * 4);                // folded 8 to 1
        w.part2 = o.take(nv_total * w.per * (FIXED_BLOCK / FOLD_GROUP / FOLD_GROUP2) * JW * 4);  // then 4 to 1
        w.vout = o.take(w.chunk * (size_t)s.m * WW * 4);     // the commitments of a chunk when the caller does not want them
        w.trst = o.take(w.chunk * 32);                        // transcript states (Fiat-Shamir mode)
        w.ch = o.take(w.chunk * (size_t)(3 + s.k) * 32);    // ... and the challenge blocks when the caller does not want them
        w.blind = o.take(w.chunk * (size_t)pb_blind_elems(s.k) * 32);   // blinding scalars expanded from the caller's key
        w.vals = w.gams = 0;
        if (mixed) {
            w.vals = o.take(w.chunk * (size_t)s.m * 8);
            w.gams = o.take(w.chunk * (size_t)s.m * 32);
        }
        w.total = o.total;
        return w;
    }

    // ---- the schedule of the argument: what the range prover and the WIP seam run behind their own first kernel -----
    // the reference's literal blinding of the argument: d_L, d_R (wip.rs:94-95), r, s, delta, eta (wip.rs:175-178); alpha and
    // amount64, the first and the last field, are the range statement's (prove_batch_device)
    static ProverConsts literals() { return ProverConsts{0, 4, 5, 33, 44, 88, 123, 0}; }
    // one chunk of `cnt` proofs in flight: shape, literals, layout and workspace, the chunk's blinding scalars (null: the
    // literals) and px entries (null: fixed strides), where records, commitments (null: none) and scalar triples go, the
    // chunk's blocks of 3 + k challenges (k_pb_fs_round / _final write e_t and e there), the stream, the window tables
    struct Chunk {
        const VerifyShape& s;
        const ProverConsts& pc;
        const ProveLayout& L;
        uint8_t* ws;
        size_t cnt;
        const uint32_t *blind, *px;
        uint32_t *o_pts, *o_V, *o_sc, *ch;
        hipStream_t st;
        const uint32_t* table;
        uint32_t* w(size_t off) const { return reinterpret_cast<uint32_t*>(ws + off); }
    };
    // one MulVec launch over `sel` of every proof's virtual proofs, then their wire points into the records
    static void mulvec(const Chunk& c, VpSel sel);
    // The chunk's blinding scalars.  slice: the chunk's part of the caller's buffer (a mixed block: gathered into w_blind
    // already), else blind_key (32 bytes, host) expanded into w_blind by k_pb_blind -- proof p of the chunk with index
    // `index` + p, or `index` + its PX_CALLER when there is a px -- else null: the literals.
    static const uint32_t* chunk_blinding(const uint32_t* slice, const uint8_t* blind_key, uint64_t index, uint32_t k, size_t cnt,
                                          const uint32_t* px, uint32_t* w_blind, hipStream_t st);
    // The argument on a chunk whose state the caller's first kernel has written (k_pb_init, k_wip_init): the k rounds and
    // the final step.  fs = false: every kernel whole, then ONE MulVec over `literal_sel`.  fs = true: each round's L_t, R_t
    // before e_t, wip.A and wip.B before e -- the kernels in halves around k + 1 MulVecs and the hashing into c.ch.
    static void argument(const Chunk& c, bool fs, VpSel literal_sel);

    // The range prover.  d_values: count x m u64 ; d_gammas: count x m scalars ; d_out_points: count x (3 + 2k) wire points ;
    // d_out_scalars: count x 3 scalars ; d_out_V: count x m wire points (may be null).
    // fs = false: the reference's constant challenges, every MulVec of the batch in ONE k_fixed_msm launch.
    // fs = true : challenges from the transcript (transcript.hpp): A and the commitments first, then y, z, then the argument
    //             -- 3 + k smaller launches.  d_out_challenges (count x (3 + k) scalars, may be null): [y, z, e, e_1..e_k].
    // Blinding (prover_batch.hpp pb_blind): d_blinding (count x (5 + 2k) canonical scalars), or blind_key (32 bytes, host)
    // expanded on the device with the global proof index index_base + p, or -- both null -- the reference's literals.
    // ps: the shape proved -- the engine's own, or a prefix view (n, m') of its tables: the proofs of PublicKey::new(n m').
    // px (one class of a mixed block, ps its view; prover_batch.hpp PX_*): `count` entries by gathered position.  The
    // values, gammas, blinding scalars and challenge blocks are then the caller's PACKED buffers and each record,
    // commitments behind it, goes to wire point PX_REC of d_out_points (d_out_V is not used).
    // d_challenges (fs = false and fixed strides alone; tu_debug.hip bpp_debug_prover_scalars): count x (3 + k) canonical
    // scalars [y, z, e, e_1..e_k], a block per proof in place of the shape's literals.  y and every e_t non-zero: the whole
    // kernels invert their product.
    static int prove_batch_device(bpp_verifier* v, const PassShape& ps, const uint64_t* d_values, const uint64_t* d_gammas,
                                  size_t count, uint64_t* d_out_points, uint64_t* d_out_scalars, uint64_t* d_out_V, bool fs,
                                  uint64_t* d_out_challenges, void* d_workspace, size_t workspace_bytes, hipStream_t st,
                                  const uint8_t* blind_key = nullptr, uint64_t index_base = 0,
                                  const uint64_t* d_blinding = nullptr, const uint32_t* px = nullptr, bool amount64 = false,
                                  const uint64_t* d_challenges = nullptr);
    static int prove_batch_device(bpp_verifier* v, const uint64_t* d_values, const uint64_t* d_gammas, size_t count,
                                  uint64_t* d_out_points, uint64_t* d_out_scalars, uint64_t* d_out_V, bool fs,
                                  uint64_t* d_out_challenges, void* d_workspace, size_t workspace_bytes, hipStream_t st,
                                  const uint8_t* blind_key = nullptr, uint64_t index_base = 0,
                                  const uint64_t* d_blinding = nullptr, bool amount64 = false) {
        return prove_batch_device(v, V::own(v), d_values, d_gammas, count, d_out_points, d_out_scalars, d_out_V, fs,
                                  d_out_challenges, d_workspace, workspace_bytes, st, blind_key, index_base, d_blinding, nullptr,
                                  amount64);
    }

    // ---- ... of a block of MIXED aggregation sizes (mixed.hpp prove_plan): proof i has m_of[i] values ---------------
    // workspace = the per-proof indices (PX_* | SX_*, by gathered position) | serialized form: the class regions of wire
    // records and the scalar triples | one class's prove_layout (the classes run one after the other on st and share it)
    struct ProveMixedLayout {
        size_t idx, records, scalars, run, total;
    };
    static ProveMixedLayout prove_mixed_layout(const bpp_verifier* v, const MixedPlan& p, size_t count, bool serialized) {
        ProveMixedLayout w;
        WsCarver o;
        w.idx = o.take(count * (size_t)(PX_WORDS + SX_WORDS) * 4);
        w.records = o.take(serialized ? p.points * WW * 4 : 0);
        w.scalars = o.take(serialized ? count * 96 : 0);
        w.run = o.take(V::class_run_max(v, p, [](const VerifyShape& s, size_t n) { return prove_layout(s, n, true).total; }));
        w.total = o.total;
        return w;
    }
    // 0 for an m_of the engine does not take
    static size_t prove_mixed_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count) {
        MixedPlan p;
        if (prove_plan(v->s, m_of, count, 0, false, p)) return 0;
        return prove_mixed_layout(v, p, count, false).total;
    }
    static size_t prove_ser_mixed_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count) {
        MixedPlan p;
        if (!V::container_shape_ok(v) || prove_plan(v->s, m_of, count, max_point_bytes<C>(), false, p)) return 0;
        return prove_mixed_layout(v, p, count, true).total;
    }
    // d_values: sum m_i u64, d_gammas: sum m_i scalars, d_blinding (may be null): 5 + 2 k_i scalars per proof, all packed
    // in caller order; m_of: host.  d_out_points: record i [A, wip.A, wip.B, L.., R.., V_0..] at wire point
    // sum_{j<i} (3 + 2 k_j + m_j) -- run_mixed's d_points; d_out_scalars: count x 3; d_out_challenges (may be null): the
    // packed 3 + k_i blocks.  Proof i's blinding index is index_base + i.  Uploads the per-proof index (blocking the host
    // until the copy has read it), the rest is enqueued on st.
    static int prove_mixed(bpp_verifier* v, const uint64_t* d_values, const uint64_t* d_gammas, const uint32_t* m_of,
                           size_t count, bool fs, const uint8_t* blind_key, uint64_t index_base, const uint64_t* d_blinding,
                           uint64_t* d_out_points, uint64_t* d_out_scalars, uint64_t* d_out_challenges, void* d_workspace,
                           size_t workspace_bytes, hipStream_t st, bool amount64 = false);
    // ... as containers packed back to back in caller order (container i of container_bytes(k_i, version) bytes) and
    // m_i encoded commitments per proof in a buffer of their own: run_serialized_mixed's input
    static int prove_serialized_mixed(bpp_verifier* v, const uint64_t* d_values, const uint64_t* d_gammas, const uint32_t* m_of,
                                      size_t count, bool fs, const uint8_t* blind_key, uint64_t index_base,
                                      const uint64_t* d_blinding, uint8_t* d_out_proofs, uint8_t* d_out_commitments,
                                      void* d_workspace, size_t workspace_bytes, hipStream_t st, uint32_t version,
                                      bool amount64 = false);
    // the shared body: plan p (with its indices) and layout L in hand, every class present proved with its view
    static int prove_mixed_classes(bpp_verifier* v, const MixedPlan& p, const ProveMixedLayout& L, const uint64_t* d_values,
                                   const uint64_t* d_gammas, bool fs, const uint8_t* blind_key, uint64_t index_base,
                                   const uint64_t* d_blinding, uint64_t* d_out_points, uint64_t* d_out_scalars,
                                   uint64_t* d_out_challenges, uint8_t* ws, size_t workspace_bytes, hipStream_t st,
                                   bool amount64 = false);

    // ---- host buffers in, host buffers out ------------------------------------------------------------------------------
    static int prove_batch(bpp_verifier* v, const uint64_t* values, const uint64_t* gammas, size_t count,
                           uint64_t* out_points, uint64_t* out_scalars, uint64_t* out_V, bool fs,
                           const uint8_t* blind_key = nullptr, uint64_t index_base = 0, bool amount64 = false);
    // bpp_range_prove_batch_mixed / _serialized_mixed past their argument checks (flags: BPP_SER_* | BPP_PROVE_AMOUNT64):
    // the device forms above between copies, the sizes of every buffer from the plan
    static int prove_mixed_host(bpp_verifier* v, const uint64_t* values, const uint64_t* gammas, const uint32_t* m_of,
                                size_t count, int flags, const uint8_t* blind_key, uint64_t index_base, uint64_t* out_points,
                                uint64_t* out_scalars, uint64_t* out_challenges);
    static int prove_serialized_mixed_host(bpp_verifier* v, const uint64_t* values, const uint64_t* gammas, const uint32_t* m_of,
                                           size_t count, int flags, const uint8_t* blind_key, uint64_t index_base,
                                           uint8_t* out_proofs, uint8_t* out_commitments);
    // the amounts (and gammas) of the block p
    static size_t plan_values(const MixedPlan& p) {
        size_t nval = 0;
        for (uint32_t c = 0; c < MIXED_CLASSES; c++) nval += p.count[c] << c;
        return nval;
    }
};

// ---- definitions: compiled by tu_prove_*.hip alone (BPP_IMPL_DEFINITIONS); everybody else sees the `extern template` below ----
#ifdef BPP_IMPL_DEFINITIONS
template <class C>
void ProveBatchImpl<C>::mulvec(const Chunk& c, VpSel sel) {
    const ProveLayout& L = c.L;
    const size_t nv = c.cnt * sel.cnt;
    // never more blocks per virtual proof than the workspace was sized for
    const unsigned per = std::min(L.per, blocks_per_proof(c.s, nv));
    launch_fixed_msm<C, 2>((unsigned)(nv * per), c.st, c.s, c.w(L.vps), c.table, c.w(L.part), per, 0u, (const uint32_t*)nullptr,
                           (uint32_t*)nullptr, (size_t)0, 0u, sel);
    // per-thread partials -> 16 -> 4 per block with every lane busy (as the verifier does); k_pb_collect adds the 4 * per left
    const size_t f1 = nv * per * (FIXED_BLOCK / FOLD_GROUP), f2 = f1 / FOLD_GROUP2;
    hipLaunchKernelGGL(k_partials_fold<C>, dim3(cdiv(f1, 64)), dim3(64), 0, c.st, c.w(L.part), FOLD_GROUP, c.w(L.part1), f1);
    hipLaunchKernelGGL(k_partials_fold<C>, dim3(cdiv(f2, 64)), dim3(64), 0, c.st, c.w(L.part1), FOLD_GROUP2, c.w(L.part2), f2);
    hipLaunchKernelGGL(k_pb_collect<C>, dim3(cdiv(nv, 64)), dim3(64), 0, c.st, c.s, sel, c.w(L.part2),
                       per * (FIXED_BLOCK / FOLD_GROUP / FOLD_GROUP2), c.o_pts, c.o_V, nv, c.px);
}

template <class C>
const uint32_t* ProveBatchImpl<C>::chunk_blinding(const uint32_t* slice, const uint8_t* blind_key, uint64_t index, uint32_t k,
                                                  size_t cnt, const uint32_t* px, uint32_t* w_blind, hipStream_t st) {
    if (slice || !blind_key) return slice;
    BlindKey bk;
    load_key_words(blind_key, bk.w);
    hipLaunchKernelGGL(k_pb_blind<C>, dim3(cdiv(cnt * pb_blind_elems(k), 64)), dim3(64), 0, st, bk, index, k, w_blind, cnt, px);
    return w_blind;
}

template <class C>
void ProveBatchImpl<C>::argument(const Chunk& c, bool fs, VpSel literal_sel) {
    const VerifyShape& s = c.s;
    const ProveLayout& L = c.L;
    const uint32_t k = s.k, nvp = pb_num_vps(k, s.m);
    const dim3 proofs((unsigned)c.cnt), lanes(cdiv(c.cnt, 64));
    auto round = [&](uint32_t t, uint32_t phase) {
        hipLaunchKernelGGL(k_pb_round<C>, proofs, dim3(256), 0, c.st, s, c.pc, c.blind, t, phase, c.w(L.a), c.w(L.b), c.w(L.cG),
                           c.w(L.cH), c.w(L.pwy), c.w(L.con), c.w(L.vps));
    };
    auto last = [&](uint32_t phase) {
        hipLaunchKernelGGL(k_pb_final<C>, proofs, dim3(256), 0, c.st, s, c.pc, c.blind, phase, c.w(L.a), c.w(L.b), c.w(L.cG),
                           c.w(L.cH), c.w(L.con), c.w(L.vps), c.o_sc, c.px);
    };
    if (!fs) {
        for (uint32_t t = 0; t < k; t++) round(t, PB_ALL);
        last(PB_ALL);
        mulvec(c, literal_sel);
        return;
    }
    for (uint32_t t = 0; t < k; t++) {
        round(t, PB_PRE);
        mulvec(c, VpSel{nvp, 1 + 2 * t, 2u, 1u});   // L_t, R_t
        hipLaunchKernelGGL(k_pb_fs_round<C>, lanes, dim3(64), 0, c.st, s, t, c.o_pts, c.w(L.trst), c.ch, c.w(L.con), c.cnt, c.px);
        round(t, PB_POST);
    }
    last(PB_PRE);
    mulvec(c, VpSel{nvp, 2 * k + 1, 2u, 1u});       // wip.A, wip.B
    hipLaunchKernelGGL(k_pb_fs_final<C>, lanes, dim3(64), 0, c.st, s, c.o_pts, c.w(L.trst), c.ch, c.w(L.con), c.cnt, c.px);
    last(PB_POST);
}

template <class C>
int ProveBatchImpl<C>::prove_batch_device(bpp_verifier* v, const PassShape& ps, const uint64_t* d_values,
                                          const uint64_t* d_gammas, size_t count, uint64_t* d_out_points,
                                          uint64_t* d_out_scalars, uint64_t* d_out_V, bool fs, uint64_t* d_out_challenges,
                                          void* d_workspace, size_t workspace_bytes, hipStream_t st, const uint8_t* blind_key,
                                          uint64_t index_base, const uint64_t* d_blinding, const uint32_t* px, bool amount64,
                                          const uint64_t* d_challenges) {
    const VerifyShape& s = ps.s;
    const uint32_t k = s.k, m = s.m, nvp = pb_num_vps(k, m);
    const ProveLayout L = prove_layout(s, count, px != nullptr);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    if (d_challenges && (fs || px)) return fail(BPP_E_ARG, "chosen challenges: literal mode, fixed strides");
    ProverConsts pc = literals();
    pc.alpha = m == 1 ? 7 : 33;         // range/mod.rs:94 / :256
    pc.amount64 = amount64 ? 1u : 0u;   // the commitments' scalar on g: the u64, not `v as i32` (range/prover.rs:37)
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    for (size_t base = 0; base < count; base += L.chunk) {
        const size_t cnt = std::min(L.chunk, count - base);
        const uint32_t* cpx = px ? px + base * PX_WORDS : nullptr;   // this chunk's entries of a mixed block
        uint32_t* o_pts = reinterpret_cast<uint32_t*>(d_out_points) + (px ? 0 : base * (size_t)(3 + 2 * k) * WW);
        uint32_t* o_sc = reinterpret_cast<uint32_t*>(d_out_scalars) + (px ? 0 : base * 24);
        uint32_t* o_V = d_out_V && !px ? reinterpret_cast<uint32_t*>(d_out_V) + base * (size_t)m * WW : W(L.vout);
        const uint64_t* vals = d_values + base * m;
        const uint32_t* gams = reinterpret_cast<const uint32_t*>(d_gammas) + base * (size_t)m * 8;
        if (px) {   // the chunk's inputs out of the caller's packed buffers
            hipLaunchKernelGGL(k_pb_gather_mixed<C>, dim3((unsigned)cnt), dim3(64), 0, st, cpx, m, k, d_values, d_gammas,
                               d_blinding, reinterpret_cast<uint64_t*>(ws + L.vals), reinterpret_cast<uint64_t*>(ws + L.gams),
                               reinterpret_cast<uint64_t*>(ws + L.blind));
            vals = reinterpret_cast<const uint64_t*>(ws + L.vals);
            gams = W(L.gams);
        }
        const uint32_t* bl = reinterpret_cast<const uint32_t*>(d_blinding);   // a mixed block's: gathered into L.blind above
        const uint32_t* blind = chunk_blinding(bl && !px ? bl + base * (size_t)pb_blind_elems(k) * 8 : bl ? W(L.blind) : nullptr,
                                               blind_key, px ? index_base : index_base + base, k, cnt, cpx, W(L.blind), st);
        // the transcript's challenges [y, z, e, e_1..e_k] are hashed into the caller's block when it has fixed strides; the
        // kernels read those, chs words apart, or the shape's literals, one block for all -- or, in their place, the blocks
        // a test chose (d_challenges)
        uint32_t* o_ch =
            d_out_challenges && !px ? reinterpret_cast<uint32_t*>(d_out_challenges) + base * (size_t)(3 + k) * 8 : W(L.ch);
        const uint32_t* chosen = reinterpret_cast<const uint32_t*>(d_challenges);
        const uint32_t* ch = fs ? o_ch : chosen ? chosen + base * (size_t)(3 + k) * 8 : ps.challenges;
        const uint32_t chs = fs || chosen ? (3 + k) * 8 : 0u;
        const Chunk c{s, pc, L, ws, cnt, blind, cpx, o_pts, o_V, o_sc, o_ch, st, v->table.u32()};
        auto init = [&](uint32_t phase) {
            hipLaunchKernelGGL(k_pb_init<C>, dim3((unsigned)cnt), dim3(256), 0, st, s, pc, blind, phase, fs ? 1u : 0u, vals, gams,
                               ch, chs, W(L.a), W(L.b), W(L.cG), W(L.cH), W(L.pwy), W(L.con), W(L.vps));
        };
        init(fs ? PB_PRE : PB_ALL);
        if (fs) {
            mulvec(c, VpSel{nvp, 0u, 1u, 1u});              // A
            mulvec(c, VpSel{nvp, 2 * k + 3, m, 1u});        // V_0 .. V_{m-1}
            hipLaunchKernelGGL(k_pb_fs_yz<C>, dim3(cdiv(cnt, 64)), dim3(64), 0, st, s, ps.tr0, o_pts, o_V, W(L.trst), o_ch, cnt,
                               cpx);
            init(PB_POST);
        }
        argument(c, fs, VpSel{nvp, 0u, nvp, 1u});   // literal mode: every virtual proof of the chunk in one launch
        if (px && d_out_challenges)   // a mixed block: the chunk's challenge blocks to their places in the packed buffer
            hipLaunchKernelGGL(k_pb_challenges_out<C>, dim3((unsigned)cnt), dim3(64), 0, st, cpx, k,
                               reinterpret_cast<const uint64_t*>(ch), chs / 2, d_out_challenges);
    }
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

// Every class present, one after the other on st, with its view and its slice of the index; the classes share L.run.
template <class C>
int ProveBatchImpl<C>::prove_mixed_classes(bpp_verifier* v, const MixedPlan& p, const ProveMixedLayout& L,
                                           const uint64_t* d_values, const uint64_t* d_gammas, bool fs, const uint8_t* blind_key,
                                           uint64_t index_base, const uint64_t* d_blinding, uint64_t* d_out_points,
                                           uint64_t* d_out_scalars, uint64_t* d_out_challenges, uint8_t* ws,
                                           size_t workspace_bytes, hipStream_t st, bool amount64) {
    const size_t count = p.px.size() / PX_WORDS;
    uint32_t* w_idx = reinterpret_cast<uint32_t*>(ws + L.idx);
    // pageable source: the copies have read it when the call returns
    HIPCHK(hipMemcpyAsync(w_idx, p.px.data(), p.px.size() * 4, hipMemcpyHostToDevice, st));
    if (!p.sidx.empty())
        HIPCHK(hipMemcpyAsync(w_idx + count * PX_WORDS, p.sidx.data(), p.sidx.size() * 4, hipMemcpyHostToDevice, st));
    for (uint32_t c = 0; c < MIXED_CLASSES; c++) {
        if (!p.count[c]) continue;
        const int rc = prove_batch_device(v, V::class_shape(v, c), d_values, d_gammas, p.count[c], d_out_points, d_out_scalars,
                                          nullptr, fs, d_out_challenges, ws + L.run, workspace_bytes - L.run, st, blind_key,
                                          index_base, d_blinding, w_idx + p.first[c] * PX_WORDS, amount64);
        if (rc) return rc;
    }
    return BPP_OK;
}

template <class C>
int ProveBatchImpl<C>::prove_mixed(bpp_verifier* v, const uint64_t* d_values, const uint64_t* d_gammas, const uint32_t* m_of,
                                   size_t count, bool fs, const uint8_t* blind_key, uint64_t index_base,
                                   const uint64_t* d_blinding, uint64_t* d_out_points, uint64_t* d_out_scalars,
                                   uint64_t* d_out_challenges, void* d_workspace, size_t workspace_bytes, hipStream_t st,
                                   bool amount64) {
    MixedPlan p;
    int rc = prove_plan(v->s, m_of, count, 0, true, p);
    if (rc) return rc;
    const ProveMixedLayout L = prove_mixed_layout(v, p, count, false);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    return prove_mixed_classes(v, p, L, d_values, d_gammas, fs, blind_key, index_base, d_blinding, d_out_points, d_out_scalars,
                               d_out_challenges, static_cast<uint8_t*>(d_workspace), workspace_bytes, st, amount64);
}

// The classes are proved into the class regions of the workspace (the layout the mixed decoder writes); the encoder is the
// only kernel that touches the caller's byte buffers.
template <class C>
int ProveBatchImpl<C>::prove_serialized_mixed(bpp_verifier* v, const uint64_t* d_values, const uint64_t* d_gammas,
                                              const uint32_t* m_of, size_t count, bool fs, const uint8_t* blind_key,
                                              uint64_t index_base, const uint64_t* d_blinding, uint8_t* d_out_proofs,
                                              uint8_t* d_out_commitments, void* d_workspace, size_t workspace_bytes,
                                              hipStream_t st, uint32_t version, bool amount64) {
    if (int rc = V::container_args_ok(v, version)) return rc;
    MixedPlan p;
    int rc = prove_plan(v->s, m_of, count, (size_t)container_point_bytes<C>(version), true, p);
    if (rc) return rc;
    const ProveMixedLayout L = prove_mixed_layout(v, p, count, true);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    rc = prove_mixed_classes(v, p, L, d_values, d_gammas, fs, blind_key, index_base, d_blinding,
                             reinterpret_cast<uint64_t*>(ws + L.records), reinterpret_cast<uint64_t*>(ws + L.scalars), nullptr, ws,
                             workspace_bytes, st, amount64);
    if (rc) return rc;
    hipLaunchKernelGGL(k_container_encode_mixed<C>, dim3((unsigned)(p.lanes / SER_WAVE)), dim3(SER_WAVE), 0, st, p.classes,
                       reinterpret_cast<const uint32_t*>(ws + L.idx) + count * PX_WORDS,
                       reinterpret_cast<const uint32_t*>(ws + L.records), reinterpret_cast<const uint32_t*>(ws + L.scalars),
                       d_out_proofs, d_out_commitments, version);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int ProveBatchImpl<C>::prove_batch(bpp_verifier* v, const uint64_t* values, const uint64_t* gammas, size_t count,
                                   uint64_t* out_points, uint64_t* out_scalars, uint64_t* out_V, bool fs,
                                   const uint8_t* blind_key, uint64_t index_base, bool amount64) {
    // (blocking copies through DevBuf where asynchronous ones on the null stream and a synchronise stood: the same
    // transfers from and to pageable host memory, in the same order around the device form's launches)
    const VerifyShape& s = v->s;
    const uint32_t k = s.k, m = s.m;
    const ProveLayout L = prove_layout(s, count);
    const size_t pts_bytes = count * (size_t)(3 + 2 * k) * WW * 4, V_bytes = count * (size_t)m * WW * 4;
    DevBuf d_val, d_gam, d_pts, d_V, d_sc, d_ws;
    HIPCHK(d_val.upload(values, count * m * 8));
    BPP_TRY(upload_scalars<C>(gammas, count * m, d_gam, nullptr));
    HIPCHK(d_pts.alloc(pts_bytes));
    HIPCHK(d_V.alloc(V_bytes));
    HIPCHK(d_sc.alloc(count * 3 * 32));
    HIPCHK(d_ws.alloc(L.total));
    BPP_TRY(prove_batch_device(v, d_val.u64(), d_gam.u64(), count, d_pts.u64(), d_sc.u64(), d_V.u64(), fs, nullptr, d_ws.p,
                               L.total, nullptr, blind_key, index_base, nullptr, amount64));
    HIPCHK(d_pts.download(out_points, pts_bytes));
    HIPCHK(d_sc.download(out_scalars, count * 96));
    if (out_V) HIPCHK(d_V.download(out_V, V_bytes));
    return BPP_OK;
}

// The plan names the proof the engine does not take; a block that only the size getter refuses (a count beyond one launch,
// an engine the container does not hold) is rejected as a whole.  The key needs the transcript, as in the device forms.
template <class C>
int ProveBatchImpl<C>::prove_mixed_host(bpp_verifier* v, const uint64_t* values, const uint64_t* gammas, const uint32_t* m_of,
                                        size_t count, int flags, const uint8_t* blind_key, uint64_t index_base,
                                        uint64_t* out_points, uint64_t* out_scalars, uint64_t* out_challenges) {
    MixedPlan p;
    if (int rc = mixed_plan(v->s, m_of, count, false, p)) return rc;
    if (count > 0x7fffffffu / 64) return fail(BPP_E_ARG, "mixed block rejected");
    const bool fs = (flags & BPP_SER_TRANSCRIPT) != 0;
    if (blind_key && !fs) return fail(BPP_E_ARG, "blinding needs BPP_SER_TRANSCRIPT");
    const size_t wsb = prove_mixed_layout(v, p, count, false).total, nval = plan_values(p);
    DevBuf dv, dg, dpts, dsc, dch, dws;
    HIPCHK(dv.upload(values, nval * 8));
    BPP_TRY(upload_scalars<C>(gammas, nval, dg, nullptr));
    HIPCHK(dpts.alloc(p.points * WW * 4));
    HIPCHK(dsc.alloc(count * 96));
    if (out_challenges) HIPCHK(dch.alloc(p.chals * 32));
    HIPCHK(dws.alloc(wsb));
    BPP_TRY(prove_mixed(v, dv.u64(), dg.u64(), m_of, count, fs, blind_key, index_base, nullptr, dpts.u64(), dsc.u64(), dch.u64(),
                        dws.p, wsb, nullptr, (flags & BPP_PROVE_AMOUNT64) != 0));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dpts.download(out_points, p.points * WW * 4));
    HIPCHK(dsc.download(out_scalars, count * 96));
    if (out_challenges) HIPCHK(dch.download(out_challenges, p.chals * 32));
    return BPP_OK;
}

template <class C>
int ProveBatchImpl<C>::prove_serialized_mixed_host(bpp_verifier* v, const uint64_t* values, const uint64_t* gammas,
                                                   const uint32_t* m_of, size_t count, int flags, const uint8_t* blind_key,
                                                   uint64_t index_base, uint8_t* out_proofs, uint8_t* out_commitments) {
    const uint32_t version = (flags & BPP_SER_UNCOMPRESSED) ? 2u : 1u;
    MixedPlan p;
    if (int rc = mixed_plan_serialized(v->s, m_of, count, (size_t)container_point_bytes<C>(version), false, p)) return rc;
    if (count > 0x7fffffffu / 64 || !prove_ser_mixed_workspace_bytes(v, m_of, count))
        return fail(BPP_E_ARG, "serialized mixed block rejected");
    const bool fs = (flags & BPP_SER_TRANSCRIPT) != 0;
    if (blind_key && !fs) return fail(BPP_E_ARG, "blinding needs BPP_SER_TRANSCRIPT");
    const size_t wsb = prove_mixed_layout(v, p, count, true).total, nval = plan_values(p);
    DevBuf dv, dg, dpr, dcm, dws;
    HIPCHK(dv.upload(values, nval * 8));
    BPP_TRY(upload_scalars<C>(gammas, nval, dg, nullptr));
    HIPCHK(dpr.alloc(p.proof_bytes));
    HIPCHK(dcm.alloc(p.comm_bytes));
    HIPCHK(dws.alloc(wsb));
    BPP_TRY(prove_serialized_mixed(v, dv.u64(), dg.u64(), m_of, count, fs, blind_key, index_base, nullptr, dpr.u8(), dcm.u8(),
                                   dws.p, wsb, nullptr, version, (flags & BPP_PROVE_AMOUNT64) != 0));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(dpr.download(out_proofs, p.proof_bytes));
    HIPCHK(dcm.download(out_commitments, p.comm_bytes));
    return BPP_OK;
}
#endif  // BPP_IMPL_DEFINITIONS

extern template struct ProveBatchImpl<Bls12381>;
extern template struct ProveBatchImpl<Secp256k1>;
extern template struct ProveBatchImpl<Ed25519>;

}  // namespace bpp
