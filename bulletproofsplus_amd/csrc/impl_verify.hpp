// impl_verify.hpp -- the batch verifier (bpp_verifier_*): window tables in HBM + one pass of the hot path
// over a device-resident batch, in its exact, mixed, serialized, combined and grouped forms.  One instantiation per curve
// (tu_verify_*.hip).  The engine's prover lives in impl_prove_batch.hpp and calls own, class_shape, class_run_max and the
// container checks of this struct.
#pragma once
#include <functional>
#include <memory>
#include <mutex>

#include "codec.hpp"
#include "combined.hpp"
#include "fixed_launch.hpp"
#include "host_util.hpp"
#include "mixed.hpp"
#include "pippenger.hpp"
#include "verify_args.hpp"

// stages of one pass, in launch order (bpp_verifier_profile reports one duration per stage)
enum { BPP_STAGE_FROM_WIRE = 0, BPP_STAGE_SCALARS, BPP_STAGE_FIXED_MSM, BPP_STAGE_VAR_MSM, BPP_STAGE_FINALIZE,
       BPP_NUM_STAGES };
constexpr int BPP_PROFILE_SLOTS = 64;  // passes remembered by the event ring

namespace bpp {
// the shape of one pass: the verifier's own (n, m), or a prefix view (n, m') of its tables (mixed.hpp)
struct PassShape {
    VerifyShape s;                // hgap = n (m - m') for a view
    const uint32_t* challenges;   // the shape's default challenges (device)
    TranscriptState tr0;          // transcript state after the domain, curve, (n, m') and the digest of the prefix key
};
}  // namespace bpp

struct bpp_verifier {
    bpp_ctx ctx;
    bpp::VerifyShape s;
    bpp::DevBuf table;       // window tables
    bpp::DevBuf challenges;  // default challenges
    bpp::TranscriptState tr0;   // transcript state after the domain, curve, (n, m) and generator digest
    // the prefix views (n, m') of the tables, m' = 1, 2, 4, .. < m (index log2 m'), and their default challenges
    std::vector<bpp::PassShape> views;
    bpp::DevBuf view_challenges;
    size_t table_bytes = 0;
    // how create filled the tables: k_tbl_fill launches, and the runs of TBL_RUN entries each generator has (reported by
    // tu_debug.hip bpp_debug_verifier_table; nothing in a pass reads them)
    uint32_t table_slabs = 0, table_runs_per_generator = 0;
    // bpp_verifier_set_subgroup_check: wire points outside the prime-order subgroup count as invalid points (off by
    // default: the in-memory API takes points that are in the group by construction, as the reference's mcl values are)
    bool check_subgroup = false;
    // optional per-stage HIP-event timing: one (begin, end) event pair per stage and remembered pass
    bool profiling = false;
    std::vector<hipEvent_t> events;  // BPP_PROFILE_SLOTS x BPP_NUM_STAGES x 2
    size_t passes_recorded = 0;
    unsigned last_blocks_per_proof = 0;
    unsigned last_horner_form = 0;   // of the last run_stage, as k_fixed_msm took it: 0, 1, 2, or 3 (the lone form of 1)
    // side stream of the lone-batch path (run(): the proof-point tables are built beside the verifier scalars), created
    // on first use
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::mutex aux_mu;   // the fork .. join of one pass is enqueued as a whole (passes of several host threads share the events)
    ~bpp_verifier() {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (aux) (void)hipStreamDestroy(aux);
    }
};

namespace bpp {

// the launch geometry of k_fixed_msm is fixed_plan.hpp's; the workspaces are sized by its blocks_per_proof
inline unsigned blocks_per_proof(const VerifyShape& s, size_t count) { return blocks_per_proof(s.NF, count); }

// The wave-per-proof (tree) Horner serves the batches too small to fill the chip: one block per proof, so that the
// chains spread over the CUs (with two tree waves per block they slowed each other down: 5.8 ms for 2 proofs against
// 4.3 ms for one).  Above HORNER_TREE_MAX proofs the one-lane-per-proof form rides beside the fixed-generator blocks.
#ifndef BPP_HORNER_TREE_MAX
#define BPP_HORNER_TREE_MAX 256
#endif
constexpr size_t HORNER_TREE_MAX = BPP_HORNER_TREE_MAX;
constexpr unsigned FOLD_GROUP = 8;    // thread partials summed by one lane of k_partials_fold (first pass)
constexpr unsigned FOLD_GROUP2 = 4;   // ... and of the second pass

struct WsLayout {
    size_t pts, bad, scalars, prep, fthread, fpart, fpart2, fpart3, vpart, vdig, vwsum, vtbl, vscr, total;
};

// the host forms of the verifier (VerifyImpl::verify_host)
enum HostForm { HOST_WIRE, HOST_MIXED, HOST_COMPRESSED, HOST_SERIALIZED, HOST_SERIALIZED_MIXED };

template <class C>
struct VerifyImpl {
    static constexpr int N = C::Fp::N;
    static constexpr int JW = jac_words<C>();
    static constexpr int WW = 2 * N + 2;
    static constexpr int PW = WW / 2;

    static WsLayout ws_layout(const VerifyShape& s, size_t count) {
        WsLayout w;
        WsCarver o;
        w.pts = o.take(count * s.NV * 2 * N * 4);
        w.bad = o.take(count * 4);
        w.scalars = o.take(count * (size_t)s.N * 32);
        w.prep = o.take(count * vs_prep_bytes<C>(s));                     // per-proof constants of the verifier-scalars kernels
        w.fthread = o.take(count * blocks_per_proof(s, count) * FIXED_BLOCK * JW * 4);                // one partial per thread
        w.fpart = o.take(count * blocks_per_proof(s, count) * (FIXED_BLOCK / FOLD_GROUP) * JW * 4);  // folded 8 to 1
        w.fpart2 = o.take(count * blocks_per_proof(s, count) * (FIXED_BLOCK / FOLD_GROUP / FOLD_GROUP2) * JW * 4);  // then 4 to 1
        w.fpart3 = o.take(count * (FIXED_BLOCK / FOLD_GROUP / FOLD_GROUP2) * JW * 4);   // then the blocks of a proof: 4 per proof
        w.vpart = o.take(count * JW * 4);                                  // one jacobian per proof
        w.vdig = o.take(count * s.NV * VAR_DIGIT_STRIDE);                 // digit bytes per proof point (65, or 2 x 33)
        w.vwsum = o.take(count * var_wsums_max<C>() * JW * 4);            // window sums
        w.vtbl = o.take(count * s.NV * VAR_MULTIPLES * 2 * N * 4);        // 1P..8P of every proof point, affine
        w.vscr = o.take(count * s.NV * 2 * (VAR_MULTIPLES - 1) * N * 4);  // Z's and their prefix products while normalising
        w.total = o.total;
        return w;
    }

    static int create(const bpp_ctx& ctx, const uint64_t* gh, const uint64_t* G, const uint64_t* H, size_t n, size_t m,
                      int window_bits, bpp_verifier** out);

    // the verifier's own shape, as a pass takes it
    static PassShape own(const bpp_verifier* v) { return PassShape{v->s, v->challenges.u32(), v->tr0}; }
    // the shape of class c (m' = 2^c) of a mixed batch: a prefix view, or the verifier's own shape
    static PassShape class_shape(const bpp_verifier* v, uint32_t c) {
        return c < v->views.size() ? v->views[c] : own(v);
    }

    // The public forms take the call as a record (verify_args.hpp VerifyArgs: the argument conventions are its fields'), the
    // workspace and the stream.  Beneath them the PassShape overloads of run and derive_challenges are the inner seam.
    // one pass over `count` proofs of shape ps (run(v, a, ...): the verifier's own)
    static int run(bpp_verifier* v, const PassShape& ps, const uint64_t* d_points, const uint64_t* d_scalars, size_t count,
                   const uint64_t* d_challenges, uint32_t* d_ok, void* d_workspace, size_t workspace_bytes,
                   uint64_t* d_out_scalars, uint64_t* d_out_result, hipStream_t st);
    static int run(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
        return run(v, own(v), a.points, a.scalars, a.count, a.challenges, a.ok, d_workspace, workspace_bytes, a.out_scalars,
                   a.out_result, st);
    }

    // the range statement's scalar stage (run, begin_pass); d_challenges null: the shape's default ones for every proof
    static int range_scalars(const PassShape& ps, const uint64_t* d_scalars, const uint64_t* d_challenges, uint32_t* w_sc,
                             size_t count, uint32_t* w_prep, hipStream_t st) {
        const uint32_t* ch = d_challenges ? reinterpret_cast<const uint32_t*>(d_challenges) : ps.challenges;
        const uint32_t ch_stride = d_challenges ? (3 + ps.s.k) * 8 : 0;
        return launch_verify_scalars<C>(ps.s, reinterpret_cast<const uint32_t*>(d_scalars), ch, ch_stride, w_sc, count, w_prep, st);
    }

    // run() with the scalar stage left to the caller: scalars(w_sc, w_prep, w_bad, st) enqueues on st whatever writes the
    // [count][s.N] MulVec scalars into w_sc (w_prep: ws_layout's per-proof scratch; w_bad: the invalid-proof flags, zeroed
    // and already marked by the wire points).  run() passes the range statement's kernels, the WIP seam (impl_wip.hpp) its own.
    using ScalarStage = std::function<int(uint32_t* w_sc, uint32_t* w_prep, uint32_t* w_bad, hipStream_t st)>;
    static int run_stage(bpp_verifier* v, const VerifyShape& s, const uint64_t* d_points, size_t count,
                         const ScalarStage& scalars, uint32_t* d_ok, void* d_workspace, size_t workspace_bytes,
                         uint64_t* d_out_scalars, uint64_t* d_out_result, hipStream_t st);

    // form of the Horner stage for a pass over `count` proofs (k_fixed_msm's horner_tree: 0, 1 or 2)
    static uint32_t horner_form(const VerifyShape& s, size_t count) {
        const bool small_job = (double)count * ((double)s.NF * fixed_adds_per_generator(s) / 7.0e9 + 9.2e-8) < 2.0e-3;
        return count <= HORNER_TREE_MAX ? 1u : (small_job ? 2u : 0u);
    }
    // The proof points' tables (k_var_tables) need the points but not the scalars: fork_tables builds them on the verifier's
    // side stream, beside whatever the caller enqueues next on `st` (the scalar kernels); join_tables makes `st` wait for them
    // (before k_var_windows).  The fork .. join of one pass is enqueued under the verifier's mutex: the side stream and its
    // two events are shared by the passes of every stream and host thread.
    static int fork_tables(bpp_verifier* v, hipStream_t st, const uint32_t* w_pts, uint32_t* w_vt, uint32_t* w_vscr, size_t items,
                           std::unique_lock<std::mutex>& lock) {
        lock = std::unique_lock<std::mutex>(v->aux_mu);
        if (!v->aux) {
            HIPCHK(hipStreamCreateWithFlags(&v->aux, hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&v->ev_fork, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&v->ev_join, hipEventDisableTiming));
        }
        HIPCHK(hipEventRecord(v->ev_fork, st));
        HIPCHK(hipStreamWaitEvent(v->aux, v->ev_fork, 0));
        hipLaunchKernelGGL(k_var_tables<C>, dim3(cdiv(items, VAR_BLOCK)), dim3(VAR_BLOCK), 0, v->aux, w_pts, w_vt, w_vscr, items);
        HIPCHK(hipEventRecord(v->ev_join, v->aux));
        return BPP_OK;
    }
    static int join_tables(bpp_verifier* v, hipStream_t st, std::unique_lock<std::mutex>& lock) {
        HIPCHK(hipStreamWaitEvent(st, v->ev_join, 0));
        lock.unlock();
        return BPP_OK;
    }
    // stage timing: ev (null when the pass is not profiled) holds ev[2 * stage] / ev[2 * stage + 1]
    static hipError_t mark(hipEvent_t* ev, int idx, hipStream_t st) { return ev ? hipEventRecord(ev[idx], st) : hipSuccess; }
    // The head of every pass (run, run_combined, grouped_begin): zero the invalid-point flags, the proof points from the
    // wire, their tables forked onto the side stream (the caller joins them before k_var_windows), the verifier scalars
    // into w_sc.  L: the pass's layout (WsLayout, CombLayout or GroupLayout), whose pts, bad, prep, vtbl and vscr it uses.
    template <class Layout>
    static int begin_pass(bpp_verifier* v, const PassShape& ps, const uint64_t* d_points, const uint64_t* d_scalars,
                          size_t count, const uint64_t* d_challenges, uint8_t* ws, const Layout& L, uint32_t* w_sc,
                          std::unique_lock<std::mutex>& aux_lock, hipStream_t st, hipEvent_t* ev);
    // ... up to the fork of the tables: everything that needs the points only
    template <class Layout>
    static int begin_points(bpp_verifier* v, const VerifyShape& s, const uint64_t* d_points, size_t count, uint8_t* ws,
                            const Layout& L, std::unique_lock<std::mutex>& aux_lock, hipStream_t st, hipEvent_t* ev);
    // The weighted checks' middle (run_combined, grouped_begin): the weights, then -- after fixed_sums(w_wt), which enqueues
    // the caller's fixed-generator sums -- the weighted proof-point scalars, their digits and, once the tables have joined,
    // `per` window sums per proof (k_var_windows with `split`).  L: CombLayout or GroupLayout.
    template <class Layout, class FixedSums>
    static int weighted_windows(bpp_verifier* v, const PassShape& ps, uint8_t* ws, const Layout& L, size_t count,
                                const uint8_t* weight_key, uint64_t index_base, const uint64_t* d_weights, uint32_t per,
                                uint32_t split, std::unique_lock<std::mutex>& aux_lock, hipStream_t st,
                                FixedSums&& fixed_sums);
    // its second half alone, for a pass whose weights exist already (run_grouped_mixed writes them once for all classes):
    // L's scalars, weights, var_sc, vdig, vtbl and vwsum
    template <class Layout>
    static int weighted_middle(bpp_verifier* v, const PassShape& ps, uint8_t* ws, const Layout& L, size_t count, uint32_t per,
                               uint32_t split, std::unique_lock<std::mutex>& aux_lock, hipStream_t st);
    // one level of k_comb_window_fold: the window sums (`per` each) of every `step` neighbouring proofs of `nrem` added
    // into one; returns how many sums per window are left
    static size_t fold_windows(const uint32_t* in, size_t nrem, uint32_t step, uint32_t* out, uint32_t per, hipStream_t st);
    static int finish(bpp_verifier* v, const VerifyShape& s, uint8_t* ws, const WsLayout& L, size_t count,
                      const uint32_t* w_sc, const uint32_t* w_vw, const uint32_t* w_bad, uint32_t* d_ok,
                      uint32_t* d_out_result, uint32_t tree, bool lone, hipStream_t st, hipEvent_t* ev);

    static int derive_challenges(bpp_verifier* v, const PassShape& ps, const uint64_t* d_points, size_t count,
                                 uint64_t* d_challenges, hipStream_t st);
    static int derive_challenges(bpp_verifier* v, const VerifyArgs& a, void*, size_t, hipStream_t st) {
        return derive_challenges(v, own(v), a.points, a.count, a.out_challenges, st);
    }

    // ---- mixed batches (mixed.hpp): proof i of shape (n, m_i), m_i a power of two <= m ---------------------------
    // the front of every mixed workspace: per-proof index | class regions of records (gathered, or decoded) | scalar triples |
    // decoder status (serialized form only) | challenges | verdicts -- all but the first two by gathered position
    struct MixedFront {
        size_t idx, pts, sc3, status, challenges, ok;
    };
    static MixedFront carve_front(WsCarver& o, const MixedPlan& p, size_t count, bool serialized) {
        MixedFront f;
        f.idx = o.take(count * (serialized ? (size_t)SX_WORDS : (size_t)MX_WORDS) * 4);
        f.pts = o.take(p.points * WW * 4);
        f.sc3 = o.take(count * 96);
        f.status = o.take(serialized ? count * 4 : 0);
        f.challenges = o.take(p.chals * 32);
        f.ok = o.take(count * 4);
        return f;
    }
    // wire form: the index upload (blocks until the copy has read it), the gather (d_scalars, d_challenges may be null)
    static int gather_front(const MixedPlan& p, const MixedFront& front, size_t count, const uint64_t* d_points,
                            const uint64_t* d_scalars, const uint64_t* d_challenges, uint8_t* ws, hipStream_t st);
    // serialized form: the index upload, then the decoder and the membership test write records, triples and status
    static int decode_front(const MixedPlan& p, const MixedFront& front, size_t count, const uint8_t* d_proofs,
                            const uint8_t* d_commitments, uint32_t version, uint8_t* ws, hipStream_t st);
    // serialized form, the way back: d_ok[caller position] = FormatError where the decoder rejected the proof, else front.ok
    static int scatter_verdicts(const MixedFront& front, uint8_t* ws, uint32_t* d_ok, size_t count, hipStream_t st);
    // one class present in a mixed batch: its shape, its gathered range and its regions of a front
    struct ClassView {
        uint32_t c;
        PassShape ps;
        size_t first, count;
        uint64_t *pts, *sc3, *challenges;
    };
    // f(view) for every class present, in ascending order, until one returns an error
    template <class F>
    static int for_each_class(const bpp_verifier* v, const MixedPlan& p, const MixedFront& front, uint8_t* ws, F&& f) {
        auto U64 = [&](size_t off) { return reinterpret_cast<uint64_t*>(ws + off); };
        for (uint32_t c = 0; c < MIXED_CLASSES; c++) {
            if (!p.count[c]) continue;
            const int rc = f(ClassView{c, class_shape(v, c), p.first[c], p.count[c], U64(front.pts) + p.pt[c] * PW,
                                       U64(front.sc3) + p.first[c] * 12, U64(front.challenges) + p.chal[c] * 4});
            if (rc) return rc;
        }
        return BPP_OK;
    }
    // the classes run one after the other on the caller's stream and share one workspace: the largest size_fn(shape, count)
    template <class F>
    static size_t class_run_max(const bpp_verifier* v, const MixedPlan& p, F&& size_fn) {
        size_t run = 0;
        for (uint32_t c = 0; c < MIXED_CLASSES; c++)
            if (p.count[c]) run = std::max<size_t>(run, size_fn(class_shape(v, c).s, p.count[c]));
        return run;
    }
    static size_t pass_bytes(const VerifyShape& s, size_t count) { return ws_layout(s, count).total; }

    // workspace = front | result points | one class pass's workspace
    struct MixedLayout {
        MixedFront f;
        size_t result, run, total;
    };
    static MixedLayout mixed_layout(const bpp_verifier* v, const MixedPlan& p, size_t count) {
        MixedLayout w;
        WsCarver o;
        w.f = carve_front(o, p, count, false);
        w.result = o.take(count * WW * 4);
        w.run = o.take(class_run_max(v, p, pass_bytes));
        w.total = o.total;
        return w;
    }
    // 0 for an m_of the verifier does not take
    static size_t mixed_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count) {
        MixedPlan p;
        if (mixed_plan(v->s, m_of, count, false, p)) return 0;
        return mixed_layout(v, p, count).total;
    }
    // Both upload the per-proof index (blocking the host until the copy has read it); the rest is enqueued on st.
    static int run_mixed(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);
    static int derive_challenges_mixed(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes,
                                       hipStream_t st);

    // ---- RangeProof::verify over SERIALIZED proofs resident in HBM (codec.hpp: the container) ---------------
    // what every serialized entry point asks of engine and container version (the size getters: of the engine alone)
    static bool container_shape_ok(const bpp_verifier* v) { return v->s.n <= 255 && v->s.m <= 255; }
    static int container_args_ok(const bpp_verifier* v, uint32_t version) {
        if (!container_shape_ok(v)) return fail(BPP_E_ARG, "the container holds n, m <= 255");
        return container_version_ok(version == 1 || version == 2 ? (size_t)container_point_bytes<C>(version) : 0);
    }
    // workspace = decoded records | scalars | decoder status | challenges (transcript mode) | run()'s workspace
    struct SerLayout {
        size_t records, scalars, status, challenges, run, total;
    };
    // group != 0: the verification behind the decoder is the grouped check (run_grouped) with groups of that size
    static SerLayout ser_layout(const VerifyShape& s, size_t count, uint32_t group = 0) {
        SerLayout w;
        WsCarver o;
        w.records = o.take(count * s.NV * WW * 4);
        w.scalars = o.take(count * 96);
        w.status = o.take(count * 4);
        w.challenges = o.take(count * (size_t)(3 + s.k) * 32);
        w.run = o.take(group ? group_layout(s, count, group).total : ws_layout(s, count).total);
        w.total = o.total;
        return w;
    }
    // Everything on `st`, no host synchronisation -- unless the record names a weight source: then the verdicts come
    // through run_grouped (synchronises `st`)
    static int run_serialized(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);

    // ---- ... of MIXED aggregation sizes: the decoder writes each record into its class region (mixed.hpp) -------
    // workspace = front (the challenges in transcript mode) | one class pass's workspace
    struct SerMixedLayout {
        MixedFront f;
        size_t run, total;
    };
    static SerMixedLayout ser_mixed_layout(const bpp_verifier* v, const MixedPlan& p, size_t count) {
        SerMixedLayout w;
        WsCarver o;
        w.f = carve_front(o, p, count, true);
        w.run = o.take(class_run_max(v, p, pass_bytes));
        w.total = o.total;
        return w;
    }
    // 0 for an m_of the verifier does not take (the larger point encoding sizes the byte-offset check)
    static size_t ser_mixed_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count,
                                            const uint32_t* outs_of = nullptr) {
        MixedPlan p;
        if (!container_shape_ok(v) || mixed_plan_serialized(v->s, m_of, count, max_point_bytes<C>(), false, p, outs_of)) return 0;
        return ser_mixed_layout(v, p, count).total;
    }
    // Uploads the per-proof index (blocking the host until the copy has read it), the rest is enqueued on st.
    static int run_serialized_mixed(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes,
                                    hipStream_t st);

    // ---- combined batch check (combined.hpp) ------------------------------------------------------------
    struct CombLayout {
        size_t pts, bad, scalars, prep, weights, comb_sc, fpart, var_sc, vdig, vtbl, vscr, vwsum, vfold, total;
        unsigned fixed_blocks;
    };
    static constexpr uint32_t COMB_FOLD_GROUP = 4;    // proofs whose window sums one lane of k_comb_window_fold adds
    static CombLayout comb_layout(const VerifyShape& s, size_t count) {
        CombLayout w;
        const size_t items = count * s.NV;
        w.fixed_blocks = blocks_per_proof(s, 1);
        WsCarver o;
        w.pts = o.take(items * 2 * N * 4);
        w.bad = o.take(count * 4);
        w.scalars = o.take(count * (size_t)s.N * 32);
        w.prep = o.take(count * vs_prep_bytes<C>(s));
        w.weights = o.take(count * 32);
        w.comb_sc = o.take((size_t)s.N * 32);
        w.fpart = o.take((size_t)(w.fixed_blocks + 1) * JW * 4);   // fixed-generator block sums + the Horner result
        w.var_sc = o.take(items * 32);
        w.vdig = o.take(items * VAR_DIGIT_STRIDE);
        w.vtbl = o.take(items * VAR_MULTIPLES * 2 * N * 4);
        w.vscr = o.take(items * 2 * (VAR_MULTIPLES - 1) * N * 4);
        w.vwsum = o.take(count * var_wsums<C>() * JW * 4);
        w.vfold = o.take((size_t)cdiv(count, COMB_FOLD_GROUP) * var_wsums<C>() * JW * 4);
        w.total = o.total;
        return w;
    }

    static int run_combined(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);

    // ---- grouped check (combined.hpp): per-proof verdicts from one weighted check per GROUP of proofs ------
    // the back of every grouped workspace, behind the proofs' window sums: their folds | per group the rows, invalid-point
    // flags, verdicts and the back end's workspace | the exact second pass's slice buffers
    struct GroupBack {
        size_t vfold, grows, gbad, gok, tail, list, x_pts, x_sc, x_ch, x_ok, x_run;
        size_t groups, slice;
    };
    static constexpr size_t GROUP_EXACT_SLICE = 2048;   // proofs of failing groups re-verified per exact pass
    static size_t exact_slice(size_t count) { return std::min<size_t>(std::max<size_t>(count, 1), GROUP_EXACT_SLICE); }
    // The exact pass runs over however many proofs the failing groups hold, and a SMALLER batch can need a LARGER
    // workspace (more blocks per proof, blocks_per_proof): room for the worst count up to the slice, of `count` proofs of s
    static size_t exact_run_max(const VerifyShape& s, size_t count) {
        size_t xrun = 0;
        for (size_t c = 1; c <= exact_slice(count); c++) xrun = std::max(xrun, ws_layout(s, c).total);
        return xrun;
    }
    // cap: the shape of the groups' rows; nv_max, k_max, xrun: the exact pass's longest record, challenge block, workspace
    static GroupBack carve_back(WsCarver& o, const VerifyShape& cap, size_t count, uint32_t group, size_t nv_max, size_t k_max,
                                size_t xrun) {
        GroupBack w;
        w.groups = cdiv(count, group);
        w.slice = exact_slice(count);
        w.vfold = o.take((size_t)cdiv(count, 2) * var_wsums<C>() * JW * 4);
        w.grows = o.take(w.groups * (size_t)cap.N * 32);
        w.gbad = o.take(w.groups * 4);
        w.gok = o.take(w.groups * 4);
        w.tail = o.take(ws_layout(cap, w.groups).total);
        w.list = o.take(w.slice * 4);
        w.x_pts = o.take(w.slice * nv_max * WW * 4);
        w.x_sc = o.take(w.slice * 96);
        w.x_ch = o.take(w.slice * (3 + k_max) * 32);
        w.x_ok = o.take(w.slice * 4);
        w.x_run = o.take(xrun);
        return w;
    }
    struct GroupLayout {
        size_t pts, bad, scalars, prep, weights, var_sc, vdig, vtbl, vscr, vwsum, total;   // per proof, as the combined check's
        GroupBack b;
    };
    static GroupLayout group_layout(const VerifyShape& s, size_t count, uint32_t group) {
        GroupLayout w;
        const size_t items = count * s.NV;
        WsCarver o;
        w.pts = o.take(items * 2 * N * 4);
        w.bad = o.take(count * 4);
        w.scalars = o.take(count * (size_t)s.N * 32);
        w.prep = o.take(count * vs_prep_bytes<C>(s));
        w.weights = o.take(count * 32);
        w.var_sc = o.take(items * 32);
        w.vdig = o.take(items * VAR_DIGIT_STRIDE);
        w.vtbl = o.take(items * VAR_MULTIPLES * 2 * N * 4);
        w.vscr = o.take(items * 2 * (VAR_MULTIPLES - 1) * N * 4);
        w.vwsum = o.take(count * var_wsums<C>() * JW * 4);
        w.b = carve_back(o, s, count, group, s.NV, s.k, exact_run_max(s, count));
        w.total = o.total;
        return w;
    }
    static int check_group(uint32_t group) {
        return group_ok(group) ? BPP_OK : fail(BPP_E_ARG, "group must be a power of two, at least 2");
    }
    // The verdict words are those bpp_verifier_run writes.  Synchronises `st`.
    static int run_grouped(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);
    // the same in two calls, so that ONE host thread can keep several batches in flight (a stream and a workspace each):
    // grouped_begin only enqueues pass 1; grouped_finish (same buffers, same stream) synchronises, reads the groups' verdicts
    // and runs pass 2.  run_grouped = begin + finish.
    static int grouped_begin(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);
    static int grouped_finish(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);
    // the grouped back end (only enqueues), behind the writers of the rows B.grows and flags B.gbad: the window sums at
    // `vwsum` (`per` per proof) folded to one set per group, the batch verifier's last stages over G virtual proofs of shape
    // cap in Horner form `tree`, each group's verdict spread over its proofs into out_verdicts
    static int group_back_end(bpp_verifier* v, const VerifyShape& cap, uint8_t* ws, const GroupBack& B, size_t vwsum,
                              uint32_t per, uint32_t tree, size_t count, uint32_t group, uint32_t* out_verdicts,
                              hipStream_t st);
    // the groups' verdicts back on the host (synchronises `st`) -> list: the positions of the failing groups' proofs,
    // ascending; h_stats (may be null): [failing groups, their proofs]
    static int failing_groups(const uint32_t* d_gok, size_t G, uint32_t group, size_t count, uint64_t* h_stats,
                              std::vector<uint32_t>& list, hipStream_t st) {
        std::vector<uint32_t> gok(G);
        HIPCHK(hipMemcpyAsync(gok.data(), d_gok, G * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        size_t failed = 0;
        for (size_t g = 0; g < G; g++)
            if (gok[g]) {
                failed++;
                for (size_t p = g * group; p < std::min(count, (g + 1) * (size_t)group); p++) list.push_back((uint32_t)p);
            }
        if (h_stats) {
            h_stats[0] = failed;
            h_stats[1] = list.size();
        }
        return BPP_OK;
    }
    // the exact second pass: the proofs (of shape ps) `list` names in src_pts, src_sc and src_ch (null: the shape's default
    // challenges) through run() a slice at a time, verdict i to out_verdicts[list[i]].  Synchronises `st` after every slice.
    static int exact_pass(bpp_verifier* v, const PassShape& ps, const uint64_t* src_pts, const uint64_t* src_sc,
                          const uint64_t* src_ch, const std::vector<uint32_t>& list, uint32_t* out_verdicts, uint8_t* ws,
                          const GroupBack& B, size_t workspace_bytes, hipStream_t st);

    // ---- grouped check over a MIXED batch (combined.hpp, mixed.hpp) -------------------------------------------
    // The PARTITION: groups are runs of `group` neighbours in GATHERED order (classes ascending, caller order within a
    // class): group g holds the gathered positions [g group, min(count, (g + 1) group)).  A group may straddle a class
    // boundary and the last one may be short; the partition is fixed by (m_of, group) before any weight is drawn, which
    // is all the soundness argument of the grouped check asks of it.  Each group is ONE virtual proof of the CAPACITY shape
    // (k_comb_fixed_grouped_mixed), so the back end (finish) runs once whatever the mix -- and costs G capacity rows
    // whatever the mix: a group of small proofs pays a full capacity row.
    // workspace = front (MixedFront, wire or serialized form) | weights and invalid-point flags by gathered position, the
    // scalars of every class, the front end's per-class buffers (shared by the classes, which run one after the other),
    // the window sums by gathered position | back (GroupBack)
    struct GroupMixedLayout {
        MixedFront f;
        size_t weights, bad, scalars, cpts, prep, var_sc, vdig, vtbl, vscr, vwsum, total;   // per proof
        size_t sc_of[MIXED_CLASSES];   // class c's scalars [count_c][N_c], from `scalars`, in bytes
        GroupBack b;
    };
    // the offsets begin_pass and weighted_middle take, for one class of the batch
    struct ClassFront {
        size_t pts, bad, prep, vtbl, vscr, scalars, weights, var_sc, vdig, vwsum;
    };
    static GroupMixedLayout group_mixed_layout(const bpp_verifier* v, const MixedPlan& p, size_t count, uint32_t group,
                                               bool serialized) {
        GroupMixedLayout w{};
        WsCarver o;
        w.f = carve_front(o, p, count, serialized);
        w.weights = o.take(count * 32);
        w.bad = o.take(count * 4);
        size_t scalars = 0, items = 0, prep = 0, xrun = 0, nv_max = 0, k_max = 0;
        for (uint32_t c = 0; c < MIXED_CLASSES; c++) {
            w.sc_of[c] = scalars;
            if (!p.count[c]) continue;
            const VerifyShape& s = class_shape(v, c).s;
            scalars += p.count[c] * (size_t)s.N * 32;
            items = std::max(items, p.count[c] * s.NV);
            prep = std::max(prep, p.count[c] * vs_prep_bytes<C>(s));
            nv_max = std::max<size_t>(nv_max, s.NV);
            k_max = std::max<size_t>(k_max, s.k);
            xrun = std::max(xrun, exact_run_max(s, p.count[c]));   // a class's exact pass runs over its own proofs
        }
        w.scalars = o.take(scalars);
        for (uint32_t c = 0; c < MIXED_CLASSES; c++) w.sc_of[c] += w.scalars;
        w.cpts = o.take(items * 2 * N * 4);
        w.prep = o.take(prep);
        w.var_sc = o.take(items * 32);
        w.vdig = o.take(items * VAR_DIGIT_STRIDE);
        w.vtbl = o.take(items * VAR_MULTIPLES * 2 * N * 4);
        w.vscr = o.take(items * 2 * (VAR_MULTIPLES - 1) * N * 4);
        w.vwsum = o.take(count * var_wsums<C>() * JW * 4);
        w.b = carve_back(o, v->s, count, group, nv_max, k_max, xrun);
        w.total = o.total;
        return w;
    }
    // 0 for an m_of or a group the verifier does not take
    static size_t grouped_mixed_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, uint32_t group) {
        MixedPlan p;
        if (!group_ok(group) || mixed_plan(v->s, m_of, count, false, p)) return 0;
        return group_mixed_layout(v, p, count, group, false).total;
    }
    static size_t ser_grouped_mixed_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, uint32_t group,
                                                    const uint32_t* outs_of = nullptr) {
        MixedPlan p;
        if (!group_ok(group) || !container_shape_ok(v) ||
            mixed_plan_serialized(v->s, m_of, count, max_point_bytes<C>(), false, p, outs_of))
            return 0;
        return group_mixed_layout(v, p, count, group, true).total;
    }
    // m_of rules and errors: run_mixed's; verdict words and the stream synchronisation: run_grouped's
    static int run_grouped_mixed(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);
    // ... behind the decoder: run_serialized_mixed's front; a container the decoder rejects keeps FormatError and fails its group
    static int run_serialized_grouped_mixed(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes,
                                            hipStream_t st);
    // the core of both, from the plan and the front L.f in the workspace (its challenges when with_challenges, its status
    // when with_status) and L.weights by gathered position: both passes; the verdicts are left in L.f.ok by GATHERED
    // position for the caller's scatter.  Synchronises `st`.
    static int grouped_mixed_core(bpp_verifier* v, const MixedPlan& p, size_t count, uint32_t group, bool with_challenges,
                                  bool with_status, uint64_t* h_stats, uint8_t* ws, const GroupMixedLayout& L,
                                  size_t workspace_bytes, hipStream_t st);

    // ---- host buffers in, host verdicts out (staging.hpp) ------------------------------------------------------------
    // bpp_range_verify_batch, _mixed, _compressed, _serialized and _serialized_mixed past their argument checks: the form's
    // device ENTRY (bpp_verifier_run, .._run_mixed, bpp_range_verify_batch_serialized[_mixed]_device) between copies, so the
    // entry's own argument rules (count per launch, flags: passed on as the caller gave them) hold here without a second
    // copy of them.  HOST_COMPRESSED: a malformed encoding, a point outside the group or a non-canonical scalar makes the
    // proof's verdict BPP_FORMAT_ERROR.
    static int verify_host(bpp_verifier* v, const VerifyArgs& a, HostForm form, int flags);

    // d_partials: n partials as bpp_verifier_run_combined wrote them (jacobian + validity word each)
    static int sum_partials(const uint32_t* d_partials, size_t n, uint32_t* d_ok, hipStream_t st);

    // Entries first .. first + count - 1 of table generator `generator` (table numbering; the caller has checked both
    // against NF and per_f, and count > 0), to host buffers: out_raw [count][2N] the device words as they are stored (one
    // copy, or null), out_wire [count][PW] the same slice through k_points_to_wire (or null).  Synchronous.
    static int table_slice(const bpp_verifier* v, uint32_t generator, uint32_t first, uint32_t count, uint32_t* out_raw,
                           uint64_t* out_wire);
};

// ---- definitions: compiled only by the translation unit that instantiates the struct (tu_*.hip defines
// BPP_IMPL_DEFINITIONS); capi.hip sees the declarations above and the `extern template` below, so it does not
// compile the kernels a second time ----
#ifdef BPP_IMPL_DEFINITIONS
template <class C>
int VerifyImpl<C>::create(const bpp_ctx& ctx, const uint64_t* gh, const uint64_t* G, const uint64_t* H, size_t n, size_t m,
                  int window_bits, bpp_verifier** out) {
    VerifyShape s;
    int rc = make_verify_shape<C>(n, m, window_bits, s);
    if (rc) return rc;
    std::vector<uint64_t> fixed((size_t)s.NF * PW);
    std::memcpy(fixed.data(), gh, 2 * PW * 8);
    std::memcpy(fixed.data() + 2 * PW, G, (size_t)s.mn * PW * 8);
    std::memcpy(fixed.data() + (size_t)(2 + s.mn) * PW, H, (size_t)s.mn * PW * 8);
    DevBuf dfixed;
    rc = upload_points<C>(fixed.data(), s.NF, dfixed, nullptr);
    if (rc) return rc;
    if constexpr (fixed_glv<C>()) {
        // the shared table evaluates [z^2] F as (beta x, -y): true in the prime-order subgroup only, and from_points-style
        // callers may hand over any curve point
        DevBuf bad;
        uint32_t hbad = 0;
        HIPCHK(bad.alloc(4));
        HIPCHK(zero_words_async(bad.p, 4, nullptr));
        hipLaunchKernelGGL(k_affm_subgroup<C>, dim3(cdiv(s.NF, 64)), dim3(64), 0, nullptr, dfixed.u32(), bad.u32(), (size_t)s.NF);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(&hbad, bad.p, 4, hipMemcpyDeviceToHost));
        if (hbad) return fail(BPP_E_ARG, "a fixed generator lies outside the prime-order subgroup");
    }
    auto v = std::make_unique<bpp_verifier>();
    v->ctx = ctx;
    v->s = s;
    const size_t entries = (size_t)s.NF * s.per_f;
    v->table_bytes = entries * 2 * N * 4;
    hipError_t e = v->table.alloc(v->table_bytes);
    if (e != hipSuccess) return fail(BPP_E_NOMEM, "window table allocation failed: ", hipGetErrorString(e));
    hipLaunchKernelGGL(k_tbl_bases<C>, dim3(cdiv(s.NF, 64)), dim3(64), 0, nullptr, s, dfixed.u32(), v->table.u32());
    // fill in slabs of generators: one thread per run of TBL_RUN entries, 2 * TBL_RUN field elements of scratch each
    const uint32_t runs_f = tbl_runs_per_generator(s);
    const uint32_t slab = (uint32_t)std::max<size_t>(1, ((size_t)1 << 21) / runs_f);
    DevBuf tbl_scratch;
    e = tbl_scratch.alloc((size_t)std::min<uint32_t>(slab, s.NF) * runs_f * 2 * TBL_RUN * N * 4);
    if (e != hipSuccess) return fail(BPP_E_NOMEM, "table scratch allocation failed: ", hipGetErrorString(e));
    for (uint32_t f0 = 0; f0 < s.NF; f0 += slab) {
        const uint32_t f1 = std::min<uint32_t>(s.NF, f0 + slab);
        const size_t total = (size_t)(f1 - f0) * runs_f;
        hipLaunchKernelGGL(k_tbl_fill<C>, dim3(cdiv(total, 64)), dim3(64), 0, nullptr, s, v->table.u32(),
                           tbl_scratch.u32(), f0, f1);
        v->table_slabs++;
    }
    v->table_runs_per_generator = runs_f;
    tr_initial_state<C>(s.n, s.m, reinterpret_cast<const uint32_t*>(fixed.data()), s.NF, v->tr0.st);
    std::vector<uint32_t> ch;
    default_challenges(s, ch);
    e = v->challenges.alloc(ch.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(v->challenges.p, ch.data(), ch.size() * 4, hipMemcpyHostToDevice);
    // the prefix views (n, m') of the same tables, m' < m (bpp_verifier_run_mixed): the prover of shape (n, m') hashes
    // its own key [g, h, G_0..G_{nm'-1}, H_0..H_{nm'-1}] and m' into the transcript, and its default challenges are
    // those of its shape
    std::vector<uint32_t> vch;
    std::vector<size_t> voff;
    for (uint32_t mp = 1; mp < s.m; mp <<= 1) {
        PassShape ps{};
        rc = make_verify_shape<C>(n, mp, window_bits, ps.s);
        if (rc) return rc;
        ps.s.hgap = s.n * (s.m - mp);
        std::vector<uint64_t> prefix((size_t)ps.s.NF * PW);
        std::memcpy(prefix.data(), fixed.data(), (size_t)(2 + ps.s.mn) * PW * 8);
        std::memcpy(prefix.data() + (size_t)(2 + ps.s.mn) * PW, fixed.data() + (size_t)(2 + s.mn) * PW,
                    (size_t)ps.s.mn * PW * 8);
        tr_initial_state<C>(ps.s.n, ps.s.m, reinterpret_cast<const uint32_t*>(prefix.data()), ps.s.NF, ps.tr0.st);
        std::vector<uint32_t> c1;
        default_challenges(ps.s, c1);
        voff.push_back(vch.size());
        vch.insert(vch.end(), c1.begin(), c1.end());
        v->views.push_back(ps);
    }
    if (e == hipSuccess && !vch.empty()) {
        e = v->view_challenges.alloc(vch.size() * 4);
        if (e == hipSuccess) e = hipMemcpy(v->view_challenges.p, vch.data(), vch.size() * 4, hipMemcpyHostToDevice);
        for (size_t i = 0; i < v->views.size(); i++) v->views[i].challenges = v->view_challenges.u32() + voff[i];
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(BPP_E_HIP, "table build failed: ", hipGetErrorString(e));
    *out = v.release();
    return BPP_OK;
}

template <class C>
int VerifyImpl<C>::table_slice(const bpp_verifier* v, uint32_t generator, uint32_t first, uint32_t count, uint32_t* out_raw,
                               uint64_t* out_wire) {
    const uint32_t* src = v->table.u32() + ((size_t)generator * v->s.per_f + first) * 2 * N;
    if (out_raw) HIPCHK(hipMemcpy(out_raw, src, (size_t)count * 2 * N * 4, hipMemcpyDeviceToHost));
    if (out_wire) {
        DevBuf dw;
        HIPCHK(dw.alloc((size_t)count * WW * 4));
        hipLaunchKernelGGL(k_points_to_wire<C>, dim3(cdiv(count, 64)), dim3(64), 0, nullptr, src, dw.u32(), (size_t)count);
        HIPCHK(hipGetLastError());
        HIPCHK(dw.download(out_wire, (size_t)count * WW * 4));
    }
    return BPP_OK;
}

template <class C>
template <class Layout>
int VerifyImpl<C>::begin_points(bpp_verifier* v, const VerifyShape& s, const uint64_t* d_points, size_t count, uint8_t* ws,
                                const Layout& L, std::unique_lock<std::mutex>& aux_lock, hipStream_t st, hipEvent_t* ev) {
    uint32_t* w_pts = reinterpret_cast<uint32_t*>(ws + L.pts);
    uint32_t* w_bad = reinterpret_cast<uint32_t*>(ws + L.bad);
    const size_t npts = count * s.NV;
    HIPCHK(zero_words_async(w_bad, count * 4, st));
    HIPCHK(mark(ev, 2 * BPP_STAGE_FROM_WIRE, st));
    hipLaunchKernelGGL(k_points_from_wire<C>, dim3(cdiv(npts, 128)), dim3(128), 0, st,
                       reinterpret_cast<const uint32_t*>(d_points), w_pts, w_bad, npts, s.NV, v->check_subgroup ? 1u : 0u);
    HIPCHK(mark(ev, 2 * BPP_STAGE_FROM_WIRE + 1, st));
    // The tables of the proof points need the points only, not the scalars -- a chain of seven additions and an inversion
    // that nothing else waits for yet -- so they are built on a side stream beside the scalar kernels and join before the
    // window sums.  For a lone batch both are latency bound; for a large one k_vs_prepare is (one lane per proof: 128 waves
    // for 8 192 proofs, 0.2 ms with the chip nearly empty) and the tables fill what it leaves.
    return fork_tables(v, st, w_pts, reinterpret_cast<uint32_t*>(ws + L.vtbl), reinterpret_cast<uint32_t*>(ws + L.vscr), npts,
                       aux_lock);
}

template <class C>
template <class Layout>
int VerifyImpl<C>::begin_pass(bpp_verifier* v, const PassShape& ps, const uint64_t* d_points, const uint64_t* d_scalars,
                              size_t count, const uint64_t* d_challenges, uint8_t* ws, const Layout& L, uint32_t* w_sc,
                              std::unique_lock<std::mutex>& aux_lock, hipStream_t st, hipEvent_t* ev) {
    int rc = begin_points(v, ps.s, d_points, count, ws, L, aux_lock, st, ev);
    if (rc) return rc;
    HIPCHK(mark(ev, 2 * BPP_STAGE_SCALARS, st));
    rc = range_scalars(ps, d_scalars, d_challenges, w_sc, count, reinterpret_cast<uint32_t*>(ws + L.prep), st);
    if (rc) return rc;
    HIPCHK(mark(ev, 2 * BPP_STAGE_SCALARS + 1, st));
    return BPP_OK;
}

template <class C>
template <class Layout, class FixedSums>
int VerifyImpl<C>::weighted_windows(bpp_verifier* v, const PassShape& ps, uint8_t* ws, const Layout& L, size_t count,
                                    const uint8_t* weight_key, uint64_t index_base, const uint64_t* d_weights, uint32_t per,
                                    uint32_t split, std::unique_lock<std::mutex>& aux_lock, hipStream_t st,
                                    FixedSums&& fixed_sums) {
    uint32_t* w_wt = reinterpret_cast<uint32_t*>(ws + L.weights);
    WeightKey wk;
    load_key_words(d_weights ? nullptr : weight_key, wk.w);
    hipLaunchKernelGGL(k_comb_weights<C>, dim3(cdiv(count, 256)), dim3(256), 0, st, wk, index_base,
                       reinterpret_cast<const uint32_t*>(d_weights), w_wt, count);
    fixed_sums(w_wt);
    return weighted_middle(v, ps, ws, L, count, per, split, aux_lock, st);
}

template <class C>
template <class Layout>
int VerifyImpl<C>::weighted_middle(bpp_verifier* v, const PassShape& ps, uint8_t* ws, const Layout& L, size_t count,
                                   uint32_t per, uint32_t split, std::unique_lock<std::mutex>& aux_lock, hipStream_t st) {
    const VerifyShape& s = ps.s;
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    uint32_t *w_sc = W(L.scalars), *w_wt = W(L.weights), *w_vs = W(L.var_sc);
    uint8_t* w_vd = ws + L.vdig;
    const size_t items = count * s.NV;
    // proof-carried points: weighted scalars -> per-proof Straus window sums (the caller sums them across proofs)
    hipLaunchKernelGGL(k_comb_var_scalars<C>, dim3(cdiv(items, 256)), dim3(256), 0, st, s, w_sc, w_wt, w_vs, items);
    hipLaunchKernelGGL(k_var_digits<C>, dim3(cdiv(items, 256)), dim3(256), 0, st, s, w_vs, w_vd, items, 1u);
    int rc = join_tables(v, st, aux_lock);
    if (rc) return rc;
    const size_t vlanes = count * per;
    hipLaunchKernelGGL(k_var_windows<C>, dim3(cdiv(vlanes, VAR_BLOCK)), dim3(VAR_BLOCK), 0, st, s, w_vd, W(L.vtbl),
                       W(L.vwsum), vlanes, split, 1u);
    return BPP_OK;
}

template <class C>
size_t VerifyImpl<C>::fold_windows(const uint32_t* in, size_t nrem, uint32_t step, uint32_t* out, uint32_t per,
                                   hipStream_t st) {
    const size_t outn = cdiv(nrem, step);
    hipLaunchKernelGGL(k_comb_window_fold<C>, dim3(cdiv(outn * per, 64)), dim3(64), 0, st, in, nrem, step, out, outn * per,
                       per);
    return outn;
}

template <class C>
int VerifyImpl<C>::run(bpp_verifier* v, const PassShape& ps, const uint64_t* d_points, const uint64_t* d_scalars,
                       size_t count, const uint64_t* d_challenges, uint32_t* d_ok, void* d_workspace,
                       size_t workspace_bytes, uint64_t* d_out_scalars, uint64_t* d_out_result, hipStream_t st) {
    return run_stage(v, ps.s, d_points, count,
                     [&](uint32_t* w_sc, uint32_t* w_prep, uint32_t*, hipStream_t st_) {
                         return range_scalars(ps, d_scalars, d_challenges, w_sc, count, w_prep, st_);
                     },
                     d_ok, d_workspace, workspace_bytes, d_out_scalars, d_out_result, st);
}

template <class C>
int VerifyImpl<C>::run_stage(bpp_verifier* v, const VerifyShape& s, const uint64_t* d_points, size_t count,
                             const ScalarStage& scalars, uint32_t* d_ok, void* d_workspace, size_t workspace_bytes,
                             uint64_t* d_out_scalars, uint64_t* d_out_result, hipStream_t st) {
    const WsLayout L = ws_layout(s, count);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    uint32_t* w_bad = reinterpret_cast<uint32_t*>(ws + L.bad);
    uint32_t* w_sc = d_out_scalars ? reinterpret_cast<uint32_t*>(d_out_scalars)
                                   : reinterpret_cast<uint32_t*>(ws + L.scalars);
    uint32_t* w_vt = reinterpret_cast<uint32_t*>(ws + L.vtbl);
    const unsigned bpp_ = blocks_per_proof(s, count);
    const size_t npts = count * s.NV;
    hipEvent_t* ev = nullptr;
    if (v->profiling) {
        ev = v->events.data() + (v->passes_recorded % BPP_PROFILE_SLOTS) * (BPP_NUM_STAGES * 2);
        v->passes_recorded++;
    }
    v->last_blocks_per_proof = bpp_;
    std::unique_lock<std::mutex> aux_lock;
    int rc = begin_points(v, s, d_points, count, ws, L, aux_lock, st, ev);
    if (rc) return rc;
    HIPCHK(mark(ev, 2 * BPP_STAGE_SCALARS, st));
    rc = scalars(w_sc, reinterpret_cast<uint32_t*>(ws + L.prep), w_bad, st);
    if (rc) return rc;
    HIPCHK(mark(ev, 2 * BPP_STAGE_SCALARS + 1, st));
    // proof-point MSM: digits, per-point tables, window sums (all arithmetic bound, so they simply run in
    // sequence); its latency-bound Horner stage rides in the first blocks of the fixed-generator launch
    uint8_t* w_vd = ws + L.vdig;
    uint32_t* w_vw = reinterpret_cast<uint32_t*>(ws + L.vwsum);
    // Horner stage (horner_form): one lane per proof (mode 0), or -- while the waves are there to spare -- one wave per
    // proof (the tree, mode 1), which reads the window sums split by scalar half (k_var_windows); in between, eight lanes
    // per proof (mode 2) while the launch would otherwise wait for the one-lane chains: the chain is ~2 ms, the eight-lane
    // form costs ~0.09 us of chip time per proof on top of the fixed-generator work (~7 G mixed additions/s) -- measured
    // on (64,1): better at 4 096 proofs, worse at 8 192
    const uint32_t tree = horner_form(s, count);
    // a launch whose blocks are all resident at once (<= FIXED_RESIDENT): only latency counts -- its blocks also sum their own
    // partials (mode 3 of k_fixed_msm) and the points of a proof are dealt to VAR_GROUPS lanes per window
    const bool lone = tree == 1 && count * bpp_ <= FIXED_RESIDENT;
    const uint32_t vgroups = lone ? VAR_GROUPS : 1u;
    v->last_horner_form = lone ? 3u : tree;
    const size_t vlanes = count * (tree == 1 ? var_wsums<C>() * vgroups : var_windows<C>());
    HIPCHK(mark(ev, 2 * BPP_STAGE_VAR_MSM, st));
    hipLaunchKernelGGL(k_var_digits<C>, dim3(cdiv(npts, 256)), dim3(256), 0, st, s, w_sc, w_vd, npts, 0u);
    rc = join_tables(v, st, aux_lock);
    if (rc) return rc;
    hipLaunchKernelGGL(k_var_windows<C>, dim3(cdiv(vlanes, VAR_BLOCK)), dim3(VAR_BLOCK), 0, st, s, w_vd, w_vt, w_vw,
                       vlanes, tree == 1 ? 1u : 0u, vgroups);
    HIPCHK(mark(ev, 2 * BPP_STAGE_VAR_MSM + 1, st));
    return finish(v, s, ws, L, count, w_sc, w_vw, w_bad, d_ok, reinterpret_cast<uint32_t*>(d_out_result), tree, lone, st,
                  ev);
}

// The rest of a pass, from the scalars [count][N] and the proof points' window sums: the fixed-generator MulVec with the
// Horner stage in its leading blocks, the folds of its partials, the verdicts.  ws / L: a workspace laid out for `count`.
template <class C>
int VerifyImpl<C>::finish(bpp_verifier* v, const VerifyShape& s, uint8_t* ws, const WsLayout& L, size_t count,
                          const uint32_t* w_sc, const uint32_t* w_vw, const uint32_t* w_bad, uint32_t* d_ok,
                          uint32_t* d_out_result, uint32_t tree, bool lone, hipStream_t st, hipEvent_t* ev) {
    // the plan (fixed_plan.hpp): bpp_ blocks per proof, but ONE for each of the first `longs` proofs of a large batch; the
    // partials stay indexed by block, nblk of them in all (<= count * bpp_, what the workspace holds)
    const FixedPlan plan = fixed_plan(s.NF, count, lone ? 3u : tree);
    const unsigned bpp_ = plan.per;
    const size_t longs = plan.long_count, shorts = count - longs, nblk = fixed_plan_blocks(plan, count);
    uint32_t* w_fp = reinterpret_cast<uint32_t*>(ws + L.fpart);
    uint32_t* w_vp = reinterpret_cast<uint32_t*>(ws + L.vpart);
    HIPCHK(mark(ev, 2 * BPP_STAGE_FIXED_MSM, st));
    const unsigned hb = tree == 1 ? (unsigned)count : cdiv(count, tree == 2 ? FIXED_BLOCK / 8 : FIXED_BLOCK);
    uint32_t* w_ft = reinterpret_cast<uint32_t*>(ws + L.fthread);
    launch_fixed_msm<C, 0>((unsigned)(hb + nblk), st, s, w_sc, v->table.u32(), w_ft, bpp_, hb, w_vw, w_vp, count,
                           lone ? 3u : tree, VpSel{1u, 0u, 1u, 0u, (uint32_t)longs});
    HIPCHK(mark(ev, 2 * BPP_STAGE_FIXED_MSM + 1, st));
    HIPCHK(mark(ev, 2 * BPP_STAGE_FINALIZE, st));
    // 128 per-thread partials per block -> 16 -> 4 (-> 4 per proof), every lane of the fold kernels busy;
    // k_finalize adds the rest
    constexpr unsigned folded1 = FIXED_BLOCK / FOLD_GROUP, per_block = folded1 / FOLD_GROUP2;   // 16, 4 per block
    const unsigned folded = bpp_ * folded1;
    uint32_t* w_fp2 = reinterpret_cast<uint32_t*>(ws + L.fpart2);
    if (tree == 1) {   // a small batch waits for latency, not throughput: one block per proof finishes the sum as a tree,
                       // over the per-block partials k_fixed_msm left (lone) or over the first fold pass's output
        if (!lone)
            hipLaunchKernelGGL(k_partials_fold<C>, dim3(cdiv(count * folded, 64)), dim3(64), 0, st, w_ft, FOLD_GROUP, w_fp,
                               count * folded);
        hipLaunchKernelGGL(k_finalize_tree<C>, dim3((unsigned)count), dim3(64), 0, st, lone ? w_ft : w_fp,
                           lone ? bpp_ : folded, w_vp, w_bad, d_ok, d_out_result, count);
        HIPCHK(mark(ev, 2 * BPP_STAGE_FINALIZE + 1, st));
        HIPCHK(hipGetLastError());
        return BPP_OK;
    }
    hipLaunchKernelGGL(k_partials_fold<C>, dim3(cdiv(nblk * folded1, 64)), dim3(64), 0, st, w_ft, FOLD_GROUP, w_fp,
                       nblk * folded1);
    // Second pass, 16 -> 4 per block.  A proof with one block is then where k_finalize wants it, so the long proofs' pass
    // writes straight into the [count][4] array that the short proofs' third pass completes: no copy, one more launch.
    uint32_t* w_fp3 = reinterpret_cast<uint32_t*>(ws + L.fpart3);
    if (longs)
        hipLaunchKernelGGL(k_partials_fold<C>, dim3(cdiv(longs * per_block, 64)), dim3(64), 0, st, w_fp, FOLD_GROUP2, w_fp3,
                           longs * per_block);
    hipLaunchKernelGGL(k_partials_fold<C>, dim3(cdiv(shorts * bpp_ * per_block, 64)), dim3(64), 0, st,
                       w_fp + longs * folded1 * JW, FOLD_GROUP2, w_fp2, shorts * bpp_ * per_block);
    const uint32_t* w_last = w_fp2;
    const unsigned last = per_block;
    if (bpp_ > 1) {   // several blocks per proof: one more pass, so that k_finalize always sees 4 partials
        hipLaunchKernelGGL(k_partials_fold<C>, dim3(cdiv(shorts * last, 64)), dim3(64), 0, st, w_fp2, bpp_,
                           w_fp3 + longs * last * JW, shorts * last);
        w_last = w_fp3;
    }
    hipLaunchKernelGGL(k_finalize<C>, dim3(cdiv(count, 64)), dim3(64), 0, st, w_last, last, w_vp, 1u, w_bad, d_ok,
                       d_out_result, count);
    HIPCHK(mark(ev, 2 * BPP_STAGE_FINALIZE + 1, st));
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int VerifyImpl<C>::run_serialized(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes,
                                  hipStream_t st) {
    const VerifyShape& s = v->s;
    const size_t count = a.count;
    const bool grouped = a.weight_key || a.weights;
    if (int rc = container_args_ok(v, a.version)) return rc;
    const SerLayout L = ser_layout(s, count, grouped ? a.group : 0u);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    uint32_t* w_rec = reinterpret_cast<uint32_t*>(ws + L.records);
    uint32_t* w_sc = reinterpret_cast<uint32_t*>(ws + L.scalars);
    uint32_t* w_st = reinterpret_cast<uint32_t*>(ws + L.status);
    uint64_t* w_ch = reinterpret_cast<uint64_t*>(ws + L.challenges);
    HIPCHK(zero_words_async(w_st, count * 4, st));
    hipLaunchKernelGGL(k_container_decode<C>, dim3(cdiv(count * s.NV, 64)), dim3(64), 0, st, s, a.proofs, a.commitments,
                       w_rec, w_sc, w_st, count, a.version);
    if constexpr (C::ID == 0)   // cofactor > 1: membership of the prime-order subgroup
        hipLaunchKernelGGL(k_records_subgroup<C>, dim3(cdiv(count * s.NV, 64)), dim3(64), 0, st, w_rec, w_st, s.NV,
                           count * s.NV);
    HIPCHK(hipGetLastError());
    VerifyArgs wire = a;   // the decoded batch: the weight source, group, verdicts and stats stay the caller's
    wire.points = reinterpret_cast<const uint64_t*>(w_rec);
    wire.scalars = reinterpret_cast<const uint64_t*>(w_sc);
    wire.challenges = a.fs ? w_ch : nullptr;
    if (a.fs) {
        int rc = derive_challenges(v, own(v), wire.points, count, w_ch, st);
        if (rc) return rc;
    }
    int rc = grouped ? run_grouped(v, wire, ws + L.run, workspace_bytes - L.run, st)
                     : run(v, wire, ws + L.run, workspace_bytes - L.run, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_container_status<C>, dim3(cdiv(count, 256)), dim3(256), 0, st, w_st, a.ok, count);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int VerifyImpl<C>::derive_challenges(bpp_verifier* v, const PassShape& ps, const uint64_t* d_points, size_t count,
                                     uint64_t* d_challenges, hipStream_t st) {
    (void)v;
    hipLaunchKernelGGL(k_transcript_challenges<C>, dim3(cdiv(count, 64)), dim3(64), 0, st, ps.s, ps.tr0,
                       reinterpret_cast<const uint32_t*>(d_points), reinterpret_cast<uint32_t*>(d_challenges), count);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int VerifyImpl<C>::gather_front(const MixedPlan& p, const MixedFront& front, size_t count, const uint64_t* d_points,
                                const uint64_t* d_scalars, const uint64_t* d_challenges, uint8_t* ws, hipStream_t st) {
    auto U64 = [&](size_t off) { return reinterpret_cast<uint64_t*>(ws + off); };
    uint32_t* w_idx = reinterpret_cast<uint32_t*>(ws + front.idx);
    // pageable source: the copy has read it when the call returns
    HIPCHK(hipMemcpyAsync(w_idx, p.idx.data(), p.idx.size() * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_mixed_gather<C>, dim3((unsigned)count), dim3(MIXED_BLOCK), 0, st, w_idx, count, d_points, d_scalars,
                       d_challenges, U64(front.pts), U64(front.sc3), U64(front.challenges));
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int VerifyImpl<C>::decode_front(const MixedPlan& p, const MixedFront& front, size_t count, const uint8_t* d_proofs,
                                const uint8_t* d_commitments, uint32_t version, uint8_t* ws, hipStream_t st) {
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    uint32_t *w_idx = W(front.idx), *w_rec = W(front.pts), *w_st = W(front.status);
    // pageable source: the copy has read it when the call returns
    HIPCHK(hipMemcpyAsync(w_idx, p.sidx.data(), p.sidx.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(zero_words_async(w_st, count * 4, st));
    const unsigned waves = (unsigned)(p.lanes / SER_WAVE);
    hipLaunchKernelGGL(k_container_decode_mixed<C>, dim3(waves), dim3(SER_WAVE), 0, st, p.classes, w_idx, d_proofs,
                       d_commitments, w_rec, W(front.sc3), w_st, version);
    if constexpr (C::ID == 0)   // cofactor > 1: membership of the prime-order subgroup
        hipLaunchKernelGGL(k_records_subgroup_mixed<C>, dim3(waves), dim3(SER_WAVE), 0, st, p.classes, w_rec, w_st);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int VerifyImpl<C>::scatter_verdicts(const MixedFront& front, uint8_t* ws, uint32_t* d_ok, size_t count, hipStream_t st) {
    auto W = [&](size_t off) { return reinterpret_cast<const uint32_t*>(ws + off); };
    hipLaunchKernelGGL(k_mixed_status_scatter<C>, dim3(cdiv(count, 256)), dim3(256), 0, st, W(front.idx), W(front.status),
                       W(front.ok), d_ok, count);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

// Gather, then today's pass over each class's contiguous region with the class's view (Horner form, lone batch and
// blocks per proof follow the class's own count), then the verdicts and result points back into caller order.
template <class C>
int VerifyImpl<C>::run_mixed(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
    const size_t count = a.count;
    MixedPlan p;
    int rc = mixed_plan(v->s, a.m_of, count, true, p);
    if (rc) return rc;
    const MixedLayout L = mixed_layout(v, p, count);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    rc = gather_front(p, L.f, count, a.points, a.scalars, a.challenges, ws, st);
    if (rc) return rc;
    uint32_t* w_ok = reinterpret_cast<uint32_t*>(ws + L.f.ok);
    uint64_t* w_res = a.out_result ? reinterpret_cast<uint64_t*>(ws + L.result) : nullptr;
    rc = for_each_class(v, p, L.f, ws, [&](const ClassView& cv) {
        return run(v, cv.ps, cv.pts, cv.sc3, cv.count, a.challenges ? cv.challenges : nullptr, w_ok + cv.first, ws + L.run,
                   workspace_bytes - L.run, nullptr, w_res ? w_res + cv.first * PW : nullptr, st);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_mixed_scatter<C>, dim3(cdiv(count, 4)), dim3(256), 0, st,
                       reinterpret_cast<const uint32_t*>(ws + L.f.idx), count, w_ok, w_res, nullptr, a.ok, a.out_result, nullptr);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int VerifyImpl<C>::derive_challenges_mixed(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes,
                                           hipStream_t st) {
    const size_t count = a.count;
    MixedPlan p;
    int rc = mixed_plan(v->s, a.m_of, count, true, p);
    if (rc) return rc;
    const MixedLayout L = mixed_layout(v, p, count);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    rc = gather_front(p, L.f, count, a.points, nullptr, nullptr, ws, st);   // the points only
    if (rc) return rc;
    rc = for_each_class(v, p, L.f, ws, [&](const ClassView& cv) {
        return derive_challenges(v, cv.ps, cv.pts, cv.count, cv.challenges, st);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_mixed_scatter<C>, dim3(cdiv(count, 4)), dim3(256), 0, st,
                       reinterpret_cast<const uint32_t*>(ws + L.f.idx), count, nullptr, nullptr,
                       reinterpret_cast<uint64_t*>(ws + L.f.challenges), nullptr, nullptr, a.out_challenges);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

// Decode into the class regions, membership test, then per class present the challenges (transcript mode) and today's
// pass with the class's view; decoder status and verdicts go back to caller order in one kernel.  A container whose
// header names another shape than m_of[i] fails the header compare of ITS class: a FormatError of that proof only.
template <class C>
int VerifyImpl<C>::run_serialized_mixed(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes,
                                        hipStream_t st) {
    const size_t count = a.count;
    if (int rc = container_args_ok(v, a.version)) return rc;
    MixedPlan p;
    int rc = mixed_plan_serialized(v->s, a.m_of, count, (size_t)container_point_bytes<C>(a.version), true, p, a.outs_of);
    if (rc) return rc;
    const SerMixedLayout L = ser_mixed_layout(v, p, count);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    rc = decode_front(p, L.f, count, a.proofs, a.commitments, a.version, ws, st);
    if (rc) return rc;
    rc = for_each_class(v, p, L.f, ws, [&](const ClassView& cv) {
        if (a.fs) {
            const int rc1 = derive_challenges(v, cv.ps, cv.pts, cv.count, cv.challenges, st);
            if (rc1) return rc1;
        }
        return run(v, cv.ps, cv.pts, cv.sc3, cv.count, a.fs ? cv.challenges : nullptr, W(L.f.ok) + cv.first, ws + L.run,
                   workspace_bytes - L.run, nullptr, nullptr, st);
    });
    if (rc) return rc;
    return scatter_verdicts(L.f, ws, a.ok, count, st);
}

template <class C>
int VerifyImpl<C>::run_combined(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
    const VerifyShape& s = v->s;
    const size_t count = a.count;
    const CombLayout L = comb_layout(s, count);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    if (count * s.NV >= ((size_t)1 << 30)) return fail(BPP_E_ARG, "count too large");
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    uint32_t* w_bad = reinterpret_cast<uint32_t*>(ws + L.bad);
    uint32_t* w_sc = reinterpret_cast<uint32_t*>(ws + L.scalars);
    uint32_t* w_cs = reinterpret_cast<uint32_t*>(ws + L.comb_sc);
    uint32_t* w_fp = reinterpret_cast<uint32_t*>(ws + L.fpart);
    HIPCHK(zero_words_async(w_cs, (size_t)s.N * 32, st));
    std::unique_lock<std::mutex> aux_lock;
    int rc = begin_pass(v, own(v), a.points, a.scalars, count, a.challenges, ws, L, w_sc, aux_lock, st, nullptr);
    if (rc) return rc;
    rc = weighted_windows(v, own(v), ws, L, count, a.weight_key, a.index_base, a.weights, var_wsums<C>(), 1u, aux_lock, st,
                          [&](const uint32_t* w_wt) {
                              hipLaunchKernelGGL(k_comb_fixed<C>, dim3(s.NF), dim3(256), 0, st, s, w_sc, w_wt, count, w_cs);
                          });
    if (rc) return rc;
    // the proofs' window sums, summed across proofs per window: 4 to 1 per level
    uint32_t* cur = reinterpret_cast<uint32_t*>(ws + L.vwsum);
    uint32_t* nxt = reinterpret_cast<uint32_t*>(ws + L.vfold);
    for (size_t nrem = count; nrem > 1; std::swap(cur, nxt))
        nrem = fold_windows(cur, nrem, COMB_FOLD_GROUP, nxt, var_wsums<C>(), st);
    // the collapsed fixed-generator MulVec (one "virtual proof") with the Horner lane over the 65 sums in its
    // leading block; the Horner result lands behind the block sums
    launch_fixed_msm<C, 1>(1 + L.fixed_blocks, st, s, w_cs, v->table.u32(), w_fp, L.fixed_blocks, 1u, cur,
                           w_fp + (size_t)L.fixed_blocks * JW, (size_t)1, 1u, VpSel{1u, 0u, 1u, 0u});
    hipLaunchKernelGGL(k_comb_sum_partials<C>, dim3(1), dim3(64), 0, st, w_fp, L.fixed_blocks + 1, (uint32_t)JW, 0u, a.ok,
                       a.out_partial);
    hipLaunchKernelGGL(k_comb_verdict<C>, dim3(1), dim3(256), 0, st, a.out_partial, w_bad, count, a.ok);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int VerifyImpl<C>::run_grouped(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
    if (int rc = grouped_begin(v, a, d_workspace, workspace_bytes, st)) return rc;
    return grouped_finish(v, a, d_workspace, workspace_bytes, st);
}

template <class C>
int VerifyImpl<C>::group_back_end(bpp_verifier* v, const VerifyShape& cap, uint8_t* ws, const GroupBack& B, size_t vwsum,
                                  uint32_t per, uint32_t tree, size_t count, uint32_t group, uint32_t* out_verdicts,
                                  hipStream_t st) {
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    uint32_t* cur = W(vwsum);
    uint32_t* nxt = W(B.vfold);
    size_t nrem = count;
    for (uint32_t left = group; left > 1; std::swap(cur, nxt)) {   // the proofs of a group are neighbours: 4 (at last 2) to 1 per level
        const uint32_t step = left >= 4 ? 4u : 2u;
        nrem = fold_windows(cur, nrem, step, nxt, per, st);
        left /= step;
    }
    int rc = finish(v, cap, ws + B.tail, ws_layout(cap, B.groups), B.groups, W(B.grows), cur, W(B.gbad), W(B.gok), nullptr, tree,
                    false, st, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_comb_group_spread, dim3(cdiv(count, 256)), dim3(256), 0, st, W(B.gok), group, out_verdicts, count);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int VerifyImpl<C>::exact_pass(bpp_verifier* v, const PassShape& ps, const uint64_t* src_pts, const uint64_t* src_sc,
                              const uint64_t* src_ch, const std::vector<uint32_t>& list, uint32_t* out_verdicts, uint8_t* ws,
                              const GroupBack& B, size_t workspace_bytes, hipStream_t st) {
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    auto U64 = [&](size_t off) { return reinterpret_cast<const uint64_t*>(ws + off); };
    const uint32_t row_pts = ps.s.NV * WW, row_sc = 24, row_ch = (3 + ps.s.k) * 8;
    for (size_t lo = 0; lo < list.size(); lo += B.slice) {
        const size_t cnt = std::min(B.slice, list.size() - lo);
        HIPCHK(hipMemcpyAsync(W(B.list), list.data() + lo, cnt * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_comb_gather_rows, dim3((unsigned)cnt), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(src_pts),
                           W(B.list), row_pts, W(B.x_pts));
        hipLaunchKernelGGL(k_comb_gather_rows, dim3((unsigned)cnt), dim3(64), 0, st, reinterpret_cast<const uint32_t*>(src_sc),
                           W(B.list), row_sc, W(B.x_sc));
        if (src_ch)
            hipLaunchKernelGGL(k_comb_gather_rows, dim3((unsigned)cnt), dim3(64), 0, st,
                               reinterpret_cast<const uint32_t*>(src_ch), W(B.list), row_ch, W(B.x_ch));
        int rc = run(v, ps, U64(B.x_pts), U64(B.x_sc), cnt, src_ch ? U64(B.x_ch) : nullptr, W(B.x_ok), ws + B.x_run,
                     workspace_bytes - B.x_run, nullptr, nullptr, st);
        if (rc) return rc;
        hipLaunchKernelGGL(k_comb_scatter_words, dim3(cdiv(cnt, 256)), dim3(256), 0, st, W(B.x_ok), W(B.list), out_verdicts, cnt);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));   // `list` slices are staged from pageable memory
    }
    return BPP_OK;
}

// pass 1 (only enqueues): one weighted check per group, through the batch verifier's own last stages at count = G
template <class C>
int VerifyImpl<C>::grouped_begin(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
    const VerifyShape& s = v->s;
    const size_t count = a.count;
    const uint32_t group = a.group;
    if (int rc = check_group(group)) return rc;
    const GroupLayout L = group_layout(s, count, group);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    if (count * s.NV >= ((size_t)1 << 30)) return fail(BPP_E_ARG, "count too large");
    if (count == 0) return BPP_OK;
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    uint32_t *w_bad = W(L.bad), *w_sc = W(L.scalars), *w_rows = W(L.b.grows), *w_gbad = W(L.b.gbad);
    const size_t G = L.b.groups;
    std::unique_lock<std::mutex> aux_lock;
    int rc = begin_pass(v, own(v), a.points, a.scalars, count, a.challenges, ws, L, w_sc, aux_lock, st, nullptr);
    if (rc) return rc;
    const uint32_t tree = horner_form(s, G);
    const uint32_t per = tree == 1 ? var_wsums<C>() : var_windows<C>();   // window sums per proof, in the layout the Horner form reads
    rc = weighted_windows(v, own(v), ws, L, count, a.weight_key, a.index_base, a.weights, per, tree == 1 ? 1u : 0u, aux_lock, st,
                          [&](const uint32_t* w_wt) {
                              hipLaunchKernelGGL(k_comb_fixed_grouped<C>, dim3((unsigned)(G * cdiv(s.NF, 64))), dim3(64), 0,
                                                 st, s, w_sc, w_wt, count, group, w_rows);
                              hipLaunchKernelGGL(k_comb_group_bad, dim3(cdiv(G, 256)), dim3(256), 0, st, w_bad, count, group,
                                                 w_gbad, G);
                          });
    if (rc) return rc;
    return group_back_end(v, s, ws, L.b, L.vwsum, per, tree, count, group, a.ok, st);
}

// the groups' verdicts come back to the host (synchronises `st`); pass 2: the proofs of the groups that failed, exactly,
// through the per-proof path.  Same buffers and stream as the grouped_begin it completes.
template <class C>
int VerifyImpl<C>::grouped_finish(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
    if (int rc = check_group(a.group)) return rc;
    const GroupLayout L = group_layout(v->s, a.count, a.group);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    if (a.stats) a.stats[0] = a.stats[1] = 0;
    if (a.count == 0) return BPP_OK;
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    std::vector<uint32_t> list;
    int rc = failing_groups(reinterpret_cast<const uint32_t*>(ws + L.b.gok), L.b.groups, a.group, a.count, a.stats, list, st);
    if (rc) return rc;
    return exact_pass(v, own(v), a.points, a.scalars, a.challenges, list, a.ok, ws, L.b, workspace_bytes, st);
}

// Pass 1: per class present, today's front end over the class's region with the class's view -- the proof points from the
// wire, their tables, the verifier scalars, the weighted proof-point scalars and their window sums, `per` per proof into ONE
// array by gathered position; then one row per group in the capacity shape's numbering, and the back end once over G virtual
// proofs of the capacity shape.  Pass 2: the proofs of the failing groups, class by class (a class's gathered range is
// contiguous), exactly, from the class regions.
template <class C>
int VerifyImpl<C>::grouped_mixed_core(bpp_verifier* v, const MixedPlan& p, size_t count, uint32_t group, bool with_challenges,
                                      bool with_status, uint64_t* h_stats, uint8_t* ws, const GroupMixedLayout& L,
                                      size_t workspace_bytes, hipStream_t st) {
    const VerifyShape& cap = v->s;
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    uint32_t *w_bad = W(L.bad), *w_ok = W(L.f.ok);
    const size_t G = L.b.groups;
    const uint32_t tree = horner_form(cap, G);
    const uint32_t per = tree == 1 ? var_wsums<C>() : var_windows<C>();   // window sums per proof, as the Horner form of G reads them
    GroupClasses gc{};
    uint32_t logm = 0;
    while ((1u << logm) < cap.m) logm++;
    gc.logn = cap.k - logm;
    for (uint32_t c = 0; c < MIXED_CLASSES; c++) {
        gc.end[c] = (uint32_t)(p.first[c] + p.count[c]);
        gc.sc[c] = (L.sc_of[c] - L.scalars) / 32;
    }
    int rc = for_each_class(v, p, L.f, ws, [&](const ClassView& cv) {
        ClassFront F;
        F.pts = L.cpts, F.prep = L.prep, F.vtbl = L.vtbl, F.vscr = L.vscr, F.var_sc = L.var_sc, F.vdig = L.vdig;
        F.bad = L.bad + cv.first * 4;
        F.scalars = L.sc_of[cv.c];
        F.weights = L.weights + cv.first * 32;
        F.vwsum = L.vwsum + cv.first * (size_t)per * JW * 4;
        std::unique_lock<std::mutex> aux_lock;
        const int rc1 = begin_pass(v, cv.ps, cv.pts, cv.sc3, cv.count, with_challenges ? cv.challenges : nullptr, ws, F,
                                   W(F.scalars), aux_lock, st, nullptr);
        if (rc1) return rc1;
        return weighted_middle(v, cv.ps, ws, F, cv.count, per, tree == 1 ? 1u : 0u, aux_lock, st);
    });
    if (rc) return rc;
    if (with_status)
        hipLaunchKernelGGL(k_comb_or_words, dim3(cdiv(count, 256)), dim3(256), 0, st, w_bad, W(L.f.status), count);
    hipLaunchKernelGGL(k_comb_fixed_grouped_mixed<C>, dim3((unsigned)(G * cdiv(cap.NF, 64))), dim3(64), 0, st, cap, gc,
                       W(L.scalars), W(L.weights), count, group, W(L.b.grows));
    hipLaunchKernelGGL(k_comb_group_bad, dim3(cdiv(G, 256)), dim3(256), 0, st, w_bad, count, group, W(L.b.gbad), G);
    rc = group_back_end(v, cap, ws, L.b, L.vwsum, per, tree, count, group, w_ok, st);
    if (rc) return rc;
    // pass 2: the failing positions, split into per class lists of positions within the class
    std::vector<uint32_t> list, redo[MIXED_CLASSES];
    rc = failing_groups(W(L.b.gok), G, group, count, h_stats, list, st);
    if (rc) return rc;
    uint32_t c = 0;
    for (uint32_t pos : list) {
        while (pos >= p.first[c] + p.count[c]) c++;
        redo[c].push_back((uint32_t)(pos - p.first[c]));
    }
    return for_each_class(v, p, L.f, ws, [&](const ClassView& cv) {
        return exact_pass(v, cv.ps, cv.pts, cv.sc3, with_challenges ? cv.challenges : nullptr, redo[cv.c], w_ok + cv.first, ws,
                          L.b, workspace_bytes, st);
    });
}

template <class C>
int VerifyImpl<C>::run_grouped_mixed(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes,
                                     hipStream_t st) {
    const size_t count = a.count;
    const uint32_t group = a.group;
    MixedPlan p;
    int rc = mixed_plan(v->s, a.m_of, count, true, p);
    if (rc) return rc;
    rc = check_group(group);
    if (rc) return rc;
    const GroupMixedLayout L = group_mixed_layout(v, p, count, group, false);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    if (a.stats) a.stats[0] = a.stats[1] = 0;
    if (count == 0) return BPP_OK;
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    uint32_t* w_idx = reinterpret_cast<uint32_t*>(ws + L.f.idx);
    rc = gather_front(p, L.f, count, a.points, a.scalars, a.challenges, ws, st);
    if (rc) return rc;
    // one lane per caller position: its weight, stored at its gathered position
    WeightKey wk;
    load_key_words(a.weights ? nullptr : a.weight_key, wk.w);
    hipLaunchKernelGGL(k_comb_weights_mixed<C>, dim3(cdiv(count, 256)), dim3(256), 0, st, wk, a.index_base,
                       reinterpret_cast<const uint32_t*>(a.weights), w_idx, (uint32_t)MX_WORDS, (uint32_t)MX_WORDS,
                       (uint32_t)MX_POS, reinterpret_cast<uint32_t*>(ws + L.weights), count);
    HIPCHK(hipGetLastError());
    rc = grouped_mixed_core(v, p, count, group, a.challenges != nullptr, false, a.stats, ws, L, workspace_bytes, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_mixed_scatter<C>, dim3(cdiv(count, 4)), dim3(256), 0, st, w_idx, count,
                       reinterpret_cast<const uint32_t*>(ws + L.f.ok), nullptr, nullptr, a.ok, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int VerifyImpl<C>::run_serialized_grouped_mixed(bpp_verifier* v, const VerifyArgs& a, void* d_workspace, size_t workspace_bytes,
                                                hipStream_t st) {
    const size_t count = a.count;
    const uint32_t group = a.group;
    if (int rc = container_args_ok(v, a.version)) return rc;
    MixedPlan p;
    int rc = mixed_plan_serialized(v->s, a.m_of, count, (size_t)container_point_bytes<C>(a.version), true, p, a.outs_of);
    if (rc) return rc;
    rc = check_group(group);
    if (rc) return rc;
    const GroupMixedLayout L = group_mixed_layout(v, p, count, group, true);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    if (a.stats) a.stats[0] = a.stats[1] = 0;
    if (count == 0) return BPP_OK;
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    rc = decode_front(p, L.f, count, a.proofs, a.commitments, a.version, ws, st);
    if (rc) return rc;
    // one lane per gathered position: the weight of its caller position
    WeightKey wk;
    load_key_words(a.weight_key, wk.w);
    hipLaunchKernelGGL(k_comb_weights_mixed<C>, dim3(cdiv(count, 256)), dim3(256), 0, st, wk, a.index_base,
                       (const uint32_t*)nullptr, W(L.f.idx), (uint32_t)SX_WORDS, (uint32_t)SX_CALLER, (uint32_t)SX_WORDS,
                       W(L.weights), count);
    HIPCHK(hipGetLastError());
    if (a.fs) {
        rc = for_each_class(v, p, L.f, ws, [&](const ClassView& cv) {
            return derive_challenges(v, cv.ps, cv.pts, cv.count, cv.challenges, st);
        });
        if (rc) return rc;
    }
    rc = grouped_mixed_core(v, p, count, group, a.fs, true, a.stats, ws, L, workspace_bytes, st);
    if (rc) return rc;
    return scatter_verdicts(L.f, ws, a.ok, count, st);
}

template <class C>
int VerifyImpl<C>::sum_partials(const uint32_t* d_partials, size_t n, uint32_t* d_ok, hipStream_t st) {
    hipLaunchKernelGGL(k_comb_sum_partials<C>, dim3(1), dim3(64), 0, st, d_partials, (uint32_t)n,
                       (uint32_t)partial_words<C>(), 1u, d_ok, (uint32_t*)nullptr);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

// 1. the byte sizes of the two inputs and of the workspace for the form, 2. upload, 3. the device entry, 4. download
template <class C>
int VerifyImpl<C>::verify_host(bpp_verifier* v, const VerifyArgs& a, HostForm form, int flags) {
    const VerifyShape& s = v->s;
    const size_t count = a.count, npts = count * s.NV, cb = (size_t)container_point_bytes<C>(a.version);
    size_t in0 = npts * WW * 4, in1 = count * 96, wsb = ws_layout(s, count).total;
    MixedPlan p;
    if (form == HOST_MIXED) {
        wsb = mixed_workspace_bytes(v, a.m_of, count);
        if (!wsb) {   // an m_i the verifier does not take: the plan names the proof
            const int rc = mixed_plan(s, a.m_of, count, false, p);
            return rc ? rc : fail(BPP_E_ARG, "mixed batch rejected");
        }
        const uint32_t logn = s.k - (uint32_t)__builtin_ctz(s.m);
        in0 = 0;
        for (size_t i = 0; i < count; i++) in0 += (size_t)(3 + 2 * (logn + (uint32_t)__builtin_ctz(a.m_of[i])) + a.m_of[i]) * WW * 4;
    } else if (form == HOST_COMPRESSED) {
        in0 = npts * compressed_bytes<C>();
    } else if (form == HOST_SERIALIZED) {
        in0 = count * container_bytes<C>(s.k, a.version), in1 = count * s.m * cb, wsb = ser_layout(s, count).total;
    } else if (form == HOST_SERIALIZED_MIXED) {
        wsb = a.outs_of ? bpp_verifier_serialized_outs_workspace_bytes(v, a.outs_of, count)
                        : bpp_verifier_serialized_mixed_workspace_bytes(v, a.m_of, count);
        const int rc = mixed_plan_serialized(s, a.m_of, count, cb, false, p, a.outs_of);   // its byte totals size the uploads
        if (rc || !wsb) return rc ? rc : fail(BPP_E_ARG, "serialized mixed batch rejected");   // an m_i the verifier does not take
        in0 = p.proof_bytes, in1 = p.comm_bytes;
    }
    DevBuf d0, d1, dok, dws, dp, dk;
    HIPCHK(d0.upload(a.points ? (const void*)a.points : a.proofs, in0));
    HIPCHK(d1.upload(a.scalars ? (const void*)a.scalars : a.commitments, in1));
    HIPCHK(dok.alloc(count * 4));
    HIPCHK(dws.alloc(wsb));
    if (form == HOST_COMPRESSED) {
        HIPCHK(dp.alloc(npts * WW * 4));
        HIPCHK(dk.alloc(npts * 4));
        // the one wire entry point for points of unknown origin besides the container: reject what is outside the
        // prime-order group too (the verifier's GLV evaluation equals s * P only there, include/bpp_amd.h)
        BPP_TRY(bpp_points_decompress_device(&v->ctx, d0.p, npts, dp.u64(), dk.u32(), 1, nullptr));
    }
    const bool flat = form == HOST_WIRE || form == HOST_COMPRESSED;
    BPP_TRY(flat ? bpp_verifier_run(v, form == HOST_WIRE ? d0.u64() : dp.u64(), d1.u64(), count, nullptr, dok.u32(), dws.p, wsb, nullptr, nullptr, nullptr)
            : form == HOST_MIXED ? bpp_verifier_run_mixed(v, d0.u64(), d1.u64(), a.m_of, count, nullptr, dok.u32(), dws.p, wsb, nullptr, nullptr)
            : form == HOST_SERIALIZED ? bpp_range_verify_batch_serialized_device(v, d0.p, d1.p, count, flags, dok.u32(), dws.p, wsb, nullptr)
            : a.outs_of ? bpp_range_verify_batch_serialized_outs_device(v, d0.p, d1.p, a.outs_of, count, flags, dok.u32(), dws.p, wsb, nullptr)
                        : bpp_range_verify_batch_serialized_mixed_device(v, d0.p, d1.p, a.m_of, count, flags, dok.u32(), dws.p, wsb, nullptr));
    HIPCHK(dok.download(a.ok, count * 4));
    if (form != HOST_COMPRESSED) return BPP_OK;
    std::vector<uint32_t> bad(npts);
    HIPCHK(dk.download(bad.data(), npts * 4));
    for (size_t i = 0; i < npts; i++)
        if (bad[i]) a.ok[i / s.NV] = BPP_FORMAT_ERROR;   // a malformed encoding / a point outside the group: ProofError::FormatError
    // ... and so does a non-canonical scalar (r', s' or delta' >= the group order): a serialized proof has one encoding
    // (little-endian host: the u64 limbs are the bytes)
    for (size_t i = 0; i < count * 3; i++)
        if (!scalar_is_canonical<C>(reinterpret_cast<const uint8_t*>(a.scalars + i * 4))) a.ok[i / 3] = BPP_FORMAT_ERROR;
    return BPP_OK;
}

#endif  // BPP_IMPL_DEFINITIONS


extern template struct VerifyImpl<Bls12381>;
extern template struct VerifyImpl<Secp256k1>;
extern template struct VerifyImpl<Ed25519>;

}  // namespace bpp
