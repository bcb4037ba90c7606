// impl_prove_batch.hpp -- the engine's batched prover (bpp_range_prove_batch*, the mixed prove entries) on a verifier's
// window tables, and the ONE schedule of the weighted inner product argument (k rounds and the final step, the MulVecs and
// the hashing between them) that it shares with the WIP seam (impl_wip.hpp).  One instantiation per curve
// (tu_prove_*.hip): the kernels of prover_batch.hpp and k_fixed_msm<C, 2> are launched from those units alone.
#pragma once
#include "impl_verify.hpp"
#include "prover_batch.hpp"

namespace bpp {

// What a prove call takes, in the C ABI's order.  For a device form the pointers are the device's, for prove_host the host's;
// m_of and blind_key (32 bytes) are the host's always.
//   m_of null : `count` proofs of the engine's own shape at fixed strides.  values: count x m u64 ; gammas: count x m scalars ;
//     blinding: count x (5 + 2k) canonical scalars.  Written: out_points, count x (3 + 2k) wire points [A, wip.A, wip.B, L..,
//     R..] ; out_scalars, count x 3 ; out_V (may be null), count x m wire points ; out_challenges (fs alone, may be null),
//     count x (3 + k) scalars [y, z, e, e_1..e_k].
//   m_of given: proof i has m_of[i] values (mixed.hpp prove_plan).  values, gammas, blinding (5 + 2 k_i scalars per proof) and
//     out_challenges (3 + k_i) are packed in caller order.  Wire form: out_points, record i [A, wip.A, wip.B, L.., R.., V_0..]
//     at wire point sum_{j<i} (3 + 2 k_j + m_j) -- run_mixed's d_points -- out_scalars, count x 3, and out_challenges (may be
//     null).  Serialized form, which out_proofs selects: out_proofs, containers packed back to back (container i of
//     container_bytes(k_i, version) bytes), and out_commitments, m_i encoded commitments per proof in a buffer of their own
//     -- run_serialized_mixed's input -- and no other output.  out_V is read by neither.
// fs = false: the reference's constant challenges, every MulVec of a chunk in ONE k_fixed_msm launch.  fs = true: challenges
// from the transcript (transcript.hpp): A and the commitments first, then y, z, then the argument -- 3 + k smaller launches.
// Blinding (prover_batch.hpp pb_blind): `blinding` (the device forms alone), or blind_key expanded on the device with proof
// i's index index_base + i, or -- both null -- the reference's literals.
struct ProveArgs {
    const uint64_t *values = nullptr, *gammas = nullptr;
    const uint32_t* m_of = nullptr;
    // the serialized form's ragged block (outs_plan.hpp), in place of m_of: proof i has outs_of[i] values and gammas and is
    // proved in the shape (n, 2^ceil(log2 outs_of[i])) over zeros in the other places; out_commitments gets outs_of[i] each
    const uint32_t* outs_of = nullptr;
    size_t count = 0;
    bool fs = false, amount64 = false;   // amount64: the commitments' scalar on g is the u64, not `v as i32`
    uint32_t version = 1;                // of the containers
    const uint8_t* blind_key = nullptr;
    uint64_t index_base = 0;
    const uint64_t* blinding = nullptr;
    uint64_t *out_points = nullptr, *out_scalars = nullptr, *out_V = nullptr, *out_challenges = nullptr;
    uint8_t *out_proofs = nullptr, *out_commitments = nullptr;
    // Not the caller's: what prove_mixed tells prove_batch_device about one class of its block, and the debug hook's challenges.
    struct Inner {
        const PassShape* ps = nullptr;   // the shape proved: a prefix view (n, m') of the engine's tables -- the proofs of
                                         // PublicKey::new(n m'); null: the engine's own
        // (device) the class's `count` entries by gathered position (prover_batch.hpp PX_*).  values, gammas, blinding and
        // out_challenges are then the block's PACKED buffers, and each record, commitments behind it, goes to wire point
        // PX_REC of out_points.
        const uint32_t* px = nullptr;
        // (device; fs = false and fixed strides alone; tu_debug.hip bpp_debug_prover_scalars) count x (3 + k) canonical
        // scalars [y, z, e, e_1..e_k], a block per proof in place of the shape's literals.  y and every e_t non-zero: the
        // whole kernels invert their product.
        const uint64_t* challenges = nullptr;
    } in;
};

template <class C>
struct ProveBatchImpl {
    using V = VerifyImpl<C>;
    static constexpr int JW = V::JW, WW = V::WW;

    // The workspace of prove_batch_device: the batch is processed in chunks of `chunk` proofs that reuse it.
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
    // The chunk's blinding scalars, c.blind.  It comes as the chunk's part of the caller's buffer (a mixed block: gathered into
    // L.blind already) and stays; null, it becomes blind_key (32 bytes, host) expanded into L.blind by k_pb_blind -- proof p
    // of the chunk with index `index` + p, or `index` + its PX_CALLER when there is a px -- or stays null: the literals.
    static void chunk_blinding(Chunk& c, const uint8_t* blind_key, uint64_t index);
    // The argument on a chunk whose state the caller's first kernel has written (k_pb_init, k_wip_init): the k rounds and
    // the final step.  fs = false: every kernel whole, then ONE MulVec over `literal_sel`.  fs = true: each round's L_t, R_t
    // before e_t, wip.A and wip.B before e -- the kernels in halves around k + 1 MulVecs and the hashing into c.ch.
    static void argument(const Chunk& c, bool fs, VpSel literal_sel);

    // ---- the device forms: every buffer of `a` and the workspace in HBM, nothing synchronises ---------------------------
    // a.m_of and a.outs_of null: prove_batch_device, else prove_mixed
    static int prove_device(bpp_verifier* v, const ProveArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
        return a.m_of || a.outs_of ? prove_mixed(v, a, d_workspace, workspace_bytes, st)
                      : prove_batch_device(v, a, d_workspace, workspace_bytes, st);
    }
    // `a.count` proofs of one shape (a.in.ps), in chunks that reuse one workspace (prove_layout)
    static int prove_batch_device(bpp_verifier* v, const ProveArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);
    // where one chunk reads its inputs and writes its outputs, and the blinding index of its first proof
    struct ChunkIo {
        const uint32_t* px;      // null: fixed strides
        const uint64_t* vals;
        const uint32_t *gams, *blinding;   // blinding: the caller's scalars for the chunk, or null
        uint64_t index;
        uint32_t *o_pts, *o_sc, *o_V, *o_ch;
    };

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
    // 0 for an m_of the engine does not take, or -- serialized -- an engine the container does not hold
    static size_t prove_mixed_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, bool serialized,
                                              const uint32_t* outs_of = nullptr) {
        MixedPlan p;
        if (serialized && !V::container_shape_ok(v)) return 0;
        if (prove_plan(v->s, m_of, count, serialized ? max_point_bytes<C>() : 0, false, p, outs_of)) return 0;
        return prove_mixed_layout(v, p, count, serialized).total;
    }
    // Every class present proved with its view, one after the other on st.  Serialized: into the class regions of the
    // workspace (the layout the mixed decoder writes); the encoder is the only kernel that touches the caller's byte buffers.
    // Uploads the per-proof index (blocking the host until the copy has read it), the rest is enqueued on st.
    static int prove_mixed(bpp_verifier* v, const ProveArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);

    // ---- host buffers in, host buffers out: prove_device on the null stream between copies, the size of every buffer from
    // the shape or from the plan; whatever output is not null is downloaded ------------------------------------------------
    static int prove_host(bpp_verifier* v, const ProveArgs& a);
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
void ProveBatchImpl<C>::chunk_blinding(Chunk& c, const uint8_t* blind_key, uint64_t index) {
    if (c.blind || !blind_key) return;
    BlindKey bk;
    load_key_words(blind_key, bk.w);
    uint32_t* w_blind = c.w(c.L.blind);
    hipLaunchKernelGGL(k_pb_blind<C>, dim3(cdiv(c.cnt * pb_blind_elems(c.s.k), 64)), dim3(64), 0, c.st, bk, index, c.s.k, w_blind,
                       c.cnt, c.px);
    c.blind = w_blind;
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
int ProveBatchImpl<C>::prove_batch_device(bpp_verifier* v, const ProveArgs& a, void* d_workspace, size_t workspace_bytes,
                                          hipStream_t st) {
    const PassShape ps = a.in.ps ? *a.in.ps : V::own(v);
    const VerifyShape& s = ps.s;
    const uint32_t k = s.k, m = s.m, nvp = pb_num_vps(k, m);
    const uint32_t* px = a.in.px;
    const ProveLayout L = prove_layout(s, a.count, px != nullptr);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    if (a.in.challenges && (a.fs || px)) return fail(BPP_E_ARG, "chosen challenges: literal mode, fixed strides");
    ProverConsts pc = literals();
    pc.alpha = m == 1 ? 7 : 33;           // range/mod.rs:94 / :256
    pc.amount64 = a.amount64 ? 1u : 0u;   // the commitments' scalar on g: the u64, not `v as i32` (range/prover.rs:37)
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    auto U32 = [](uint64_t* q) { return reinterpret_cast<uint32_t*>(q); };
    auto CU32 = [](const uint64_t* q) { return reinterpret_cast<const uint32_t*>(q); };
    const size_t rec = (size_t)(3 + 2 * k) * WW, chal = (size_t)(3 + k) * 8, bl = (size_t)pb_blind_elems(k) * 8;   // words
    for (size_t base = 0; base < a.count; base += L.chunk) {
        const size_t cnt = std::min(L.chunk, a.count - base);
        ChunkIo io;
        if (px) {
            // One class of a mixed block.  The chunk's inputs are gathered out of the caller's packed buffers; records
            // (commitments behind them), triples and challenge blocks go through the index, whose PX_CALLER carries the
            // proof's part of the blinding index.
            const uint32_t* cpx = px + base * PX_WORDS;
            uint64_t* g_vals = reinterpret_cast<uint64_t*>(ws + L.vals);
            hipLaunchKernelGGL(k_pb_gather_mixed<C>, dim3((unsigned)cnt), dim3(64), 0, st, cpx, m, k, a.values, a.gammas,
                               a.blinding, g_vals, reinterpret_cast<uint64_t*>(ws + L.gams),
                               reinterpret_cast<uint64_t*>(ws + L.blind));
            io = ChunkIo{cpx, g_vals, W(L.gams), a.blinding ? W(L.blind) : nullptr, a.index_base, U32(a.out_points),
                         U32(a.out_scalars), W(L.vout), W(L.ch)};
        } else {
            // Fixed strides: the chunk's slice of every buffer; the commitments and the challenge blocks that the caller
            // does not want stay in the workspace.
            io = ChunkIo{nullptr,
                         a.values + base * m,
                         CU32(a.gammas) + base * (size_t)m * 8,
                         a.blinding ? CU32(a.blinding) + base * bl : nullptr,
                         a.index_base + base,
                         U32(a.out_points) + base * rec,
                         U32(a.out_scalars) + base * 24,
                         a.out_V ? U32(a.out_V) + base * (size_t)m * WW : W(L.vout),
                         a.out_challenges ? U32(a.out_challenges) + base * chal : W(L.ch)};
        }
        Chunk c{s, pc, L, ws, cnt, io.blinding, io.px, io.o_pts, io.o_V, io.o_sc, io.o_ch, st, v->table.u32()};
        chunk_blinding(c, a.blind_key, io.index);
        // the transcript's challenges [y, z, e, e_1..e_k] are hashed into io.o_ch; the kernels read those, chs words apart,
        // or the shape's literals, one block for all -- or, in their place, the blocks a test chose (a.in.challenges)
        const uint32_t* chosen = a.in.challenges ? CU32(a.in.challenges) + base * chal : nullptr;
        const uint32_t* ch = a.fs ? io.o_ch : chosen ? chosen : ps.challenges;
        const uint32_t chs = a.fs || chosen ? (uint32_t)chal : 0u;
        auto init = [&](uint32_t phase) {
            hipLaunchKernelGGL(k_pb_init<C>, dim3((unsigned)cnt), dim3(256), 0, st, s, pc, c.blind, phase, a.fs ? 1u : 0u, io.vals,
                               io.gams, ch, chs, W(L.a), W(L.b), W(L.cG), W(L.cH), W(L.pwy), W(L.con), W(L.vps));
        };
        init(a.fs ? PB_PRE : PB_ALL);
        if (a.fs) {
            mulvec(c, VpSel{nvp, 0u, 1u, 1u});              // A
            mulvec(c, VpSel{nvp, 2 * k + 3, m, 1u});        // V_0 .. V_{m-1}
            hipLaunchKernelGGL(k_pb_fs_yz<C>, dim3(cdiv(cnt, 64)), dim3(64), 0, st, s, ps.tr0, io.o_pts, io.o_V, W(L.trst),
                               io.o_ch, cnt, io.px);
            init(PB_POST);
        }
        argument(c, a.fs, VpSel{nvp, 0u, nvp, 1u});   // literal mode: every virtual proof of the chunk in one launch
        if (px && a.out_challenges)   // a mixed block: the chunk's challenge blocks to their places in the packed buffer
            hipLaunchKernelGGL(k_pb_challenges_out<C>, dim3((unsigned)cnt), dim3(64), 0, st, io.px, k,
                               reinterpret_cast<const uint64_t*>(ch), chs / 2, a.out_challenges);
    }
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int ProveBatchImpl<C>::prove_mixed(bpp_verifier* v, const ProveArgs& a, void* d_workspace, size_t workspace_bytes,
                                   hipStream_t st) {
    const bool serialized = a.out_proofs != nullptr;
    if (serialized) BPP_TRY(V::container_args_ok(v, a.version));
    const size_t count = a.count;
    MixedPlan p;
    BPP_TRY(prove_plan(v->s, a.m_of, count, serialized ? (size_t)container_point_bytes<C>(a.version) : 0, true, p, a.outs_of));
    const ProveMixedLayout L = prove_mixed_layout(v, p, count, serialized);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    uint32_t* w_idx = reinterpret_cast<uint32_t*>(ws + L.idx);
    // pageable source: the copies have read it when the call returns, so the plan need only outlive these two enqueues
    HIPCHK(hipMemcpyAsync(w_idx, p.px.data(), p.px.size() * 4, hipMemcpyHostToDevice, st));
    if (!p.sidx.empty())
        HIPCHK(hipMemcpyAsync(w_idx + count * PX_WORDS, p.sidx.data(), p.sidx.size() * 4, hipMemcpyHostToDevice, st));
    // what every class is told: the block's packed inputs and, of the outputs, what the index leads to
    ProveArgs cls = a;
    cls.m_of = cls.outs_of = nullptr;
    cls.out_V = nullptr;
    cls.out_proofs = cls.out_commitments = nullptr;
    if (serialized) {
        cls.out_points = reinterpret_cast<uint64_t*>(ws + L.records);
        cls.out_scalars = reinterpret_cast<uint64_t*>(ws + L.scalars);
        cls.out_challenges = nullptr;
    }
    for (uint32_t c = 0; c < MIXED_CLASSES; c++) {
        if (!p.count[c]) continue;
        const PassShape ps = V::class_shape(v, c);
        cls.count = p.count[c];
        cls.in.ps = &ps;
        cls.in.px = w_idx + p.first[c] * PX_WORDS;
        BPP_TRY(prove_batch_device(v, cls, ws + L.run, workspace_bytes - L.run, st));
    }
    if (!serialized) return BPP_OK;
    hipLaunchKernelGGL(k_container_encode_mixed<C>, dim3((unsigned)(p.lanes / SER_WAVE)), dim3(SER_WAVE), 0, st, p.classes,
                       w_idx + count * PX_WORDS, reinterpret_cast<const uint32_t*>(ws + L.records),
                       reinterpret_cast<const uint32_t*>(ws + L.scalars), a.out_proofs, a.out_commitments, a.version);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

// Staged as staging.hpp says.  A mixed block: the plan names the proof the engine does not take; a block that only the size
// getter refuses (a count beyond one launch, an engine the container does not hold) is rejected as a whole, and the key
// needs the transcript, as in the device entries.  hipDeviceSynchronize stands ahead of the downloads for every form.
template <class C>
int ProveBatchImpl<C>::prove_host(bpp_verifier* v, const ProveArgs& a) {
    const VerifyShape& s = v->s;
    const size_t count = a.count;
    const bool serialized = a.out_proofs != nullptr;
    if (a.blinding) return fail(BPP_E_ARG, "the host forms take blind_key, not blinding scalars");
    // a block at fixed strides, then a mixed one: amounts, wire points, challenges, workspace bytes
    size_t nval = count * s.m, points = count * (size_t)(3 + 2 * s.k), chals = count * (size_t)(3 + s.k), wsb = 0;
    MixedPlan p;
    if (a.m_of || a.outs_of) {
        BPP_TRY(serialized ? mixed_plan_serialized(s, a.m_of, count, (size_t)container_point_bytes<C>(a.version), false, p, a.outs_of)
                           : mixed_plan(s, a.m_of, count, false, p));
        if (count > 0x7fffffffu / 64 || (serialized && !prove_mixed_workspace_bytes(v, a.m_of, count, true, a.outs_of)))
            return fail(BPP_E_ARG, serialized ? "serialized mixed block rejected" : "mixed block rejected");
        nval = 0;
        for (uint32_t c = 0; c < MIXED_CLASSES; c++) nval += p.count[c] << c;
        if (a.outs_of) nval = p.n_out;   // a ragged block: the values and gammas of the outputs there are
        points = p.points;
        chals = p.chals;
        wsb = prove_mixed_layout(v, p, count, serialized).total;
    } else {
        wsb = prove_layout(s, count).total;
    }
    if (a.blind_key && !a.fs) return fail(BPP_E_ARG, "blinding needs BPP_SER_TRANSCRIPT");
    struct Out {
        void* host;
        size_t bytes;
        DevBuf d;
    } outs[] = {{a.out_points, points * WW * 4}, {a.out_scalars, count * 96},    {a.out_V, count * (size_t)s.m * WW * 4},
                {a.out_challenges, chals * 32}, {a.out_proofs, p.proof_bytes}, {a.out_commitments, p.comm_bytes}};
    DevBuf dv, dg, dws;
    HIPCHK(dv.upload(a.values, nval * 8));
    BPP_TRY(upload_scalars<C>(a.gammas, nval, dg, nullptr));
    for (Out& o : outs)
        if (o.host) HIPCHK(o.d.alloc(o.bytes));
    HIPCHK(dws.alloc(wsb));
    ProveArgs d = a;
    d.values = dv.u64(); d.gammas = dg.u64();
    d.out_points = outs[0].d.u64(); d.out_scalars = outs[1].d.u64(); d.out_V = outs[2].d.u64();
    d.out_challenges = outs[3].d.u64(); d.out_proofs = outs[4].d.u8(); d.out_commitments = outs[5].d.u8();
    BPP_TRY(prove_device(v, d, dws.p, wsb, nullptr));
    HIPCHK(hipDeviceSynchronize());
    for (Out& o : outs)
        if (o.host) HIPCHK(o.d.download(o.host, o.bytes));
    return BPP_OK;
}
#endif  // BPP_IMPL_DEFINITIONS

extern template struct ProveBatchImpl<Bls12381>;
extern template struct ProveBatchImpl<Secp256k1>;
extern template struct ProveBatchImpl<Ed25519>;

}  // namespace bpp
