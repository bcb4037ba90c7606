// capi.hip -- the extern "C" boundary of libbpp_amd.so (declared in include/bpp_amd.h).  Thin: argument
// checks, the entry shim, curve dispatch, then the per-curve implementations (impl_*.hpp, compiled in tu_*.hip) and the
// literal single-call API (literal.hpp).  The verifier's, the prover's and the receiver's entries fill an argument record and
// pass ONE check each (verify_args.hpp verify_args; prove_args below; scan_args.hpp scan_args for recovery and the scans,
// find_args for verify-and-find), which hold what tells their entries apart as data.  No buffer is
// staged here: the host forms live in the *Impl<C> structs as *_host.
// No CPU fallback: every entry point launches HIP kernels on the context's device.
#include "codec.hpp"
#include "commit.hpp"
#include "container_scan.hpp"
#include "impl_msm.hpp"
#include "impl_prove.hpp"
#include "impl_prove_batch.hpp"
#include "impl_verify.hpp"
#include "impl_wip.hpp"
#include "literal.hpp"
#include "recover.hpp"
#include "find.hpp"
#include "outputs.hpp"
#include "recover_keys.hpp"

using namespace bpp;

namespace {
// The entry shims.  Every entry point past its argument checks runs here: under guarded (abi_guard.hpp), so nothing
// unwinds across the C ABI, with the caller count `c` bounded before anything is read, laid out, allocated or launched.
// on_device runs f() on a device; on_ctx runs the calls of a context -- or of a verifier, through its copy v->ctx -- on
// its device (a verifier's launches must go to the device that holds its tables) as f(curve tag) on the curve's
// implementation.
template <class F>
int on_device(int device, Count c, F&& f) noexcept {
    return guarded(c, [&]() -> int {
        HIPCHK(hipSetDevice(device));
        return f();
    });
}
template <class F>
int on_device(int device, F&& f) noexcept {
    return on_device(device, Count{0, ""}, f);
}
template <class F>
int on_ctx(const bpp_ctx& ctx, Count c, F&& f) noexcept {
    return on_device(ctx.device, c, [&] { return dispatch(ctx.curve, f); });
}
template <class F>
int on_ctx(const bpp_ctx& ctx, F&& f) noexcept {
    return on_ctx(ctx, Count{0, ""}, f);
}
// the size getters: f(curve tag), or 0 for a null handle or an exception
template <class F>
size_t size_for(const bpp_ctx* ctx, F&& f) noexcept {
    size_t r = 0;
    if (ctx)
        (void)guarded([&] {
            return dispatch(ctx->curve, [&](auto cv) -> int {
                r = f(cv);
                return 0;
            });
        });
    return r;
}
template <class F>
size_t size_for(const bpp_verifier* v, F&& f) {
    return size_for(v ? &v->ctx : nullptr, f);
}
// The verifier entries: each fills its record in the C ABI's order and passes verify_args (verify_args.hpp), which is told
// this much of the handle and answers an empty batch itself.
VerifierFacts facts(const bpp_verifier* v) { return v ? VerifierFacts{true, v->ctx.curve, v->s.n, v->s.m} : VerifierFacts{}; }
static_assert(SCAN_ANSWERED == VERIFY_ANSWERED, "answered() serves verify_args and scan_args");
int answered(int rc) { return rc == VERIFY_ANSWERED ? BPP_OK : rc; }
hipStream_t hip(void* stream) { return static_cast<hipStream_t>(stream); }
// mean milliseconds per stage over the first `passes` passes of an event ring: pass p's stage t runs from
// ev[p * per_pass + t * step] to the event after it
int stage_means(const hipEvent_t* ev, size_t passes, size_t per_pass, int stages, int step, float* out_ms) {
    for (int t = 0; t < stages; t++) out_ms[t] = 0.f;
    for (size_t p = 0; p < passes; p++)
        for (int t = 0; t < stages; t++) {
            const hipEvent_t* e = ev + p * per_pass + t * step;
            HIPCHK(hipEventSynchronize(e[1]));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, e[0], e[1]));
            out_ms[t] += ms;
        }
    for (int t = 0; t < stages; t++) out_ms[t] = passes ? out_ms[t] / (float)passes : 0.f;
    return BPP_OK;
}
}  // namespace

extern "C" const char* bpp_last_error(void) { return last_error(); }

extern "C" int bpp_init(int curve_id, int device, bpp_ctx** out_ctx) {
    if (!out_ctx) return fail(BPP_E_ARG, "null out_ctx");
    if (curve_id != BPP_BLS12_381_G1 && curve_id != BPP_SECP256K1 && curve_id != BPP_ED25519)
        return fail(BPP_E_ARG, "unknown curve id");
    return guarded([&]() -> int {
        int ndev = 0;
        HIPCHK(hipGetDeviceCount(&ndev));
        if (device < 0 || device >= ndev) return fail(BPP_E_HIP, "no such HIP device");
        return on_device(device, [&] {
            *out_ctx = new bpp_ctx{curve_id, device};
            return BPP_OK;
        });
    });
}
extern "C" void bpp_destroy(bpp_ctx* ctx) {
    if (!ctx) return;
    for (hipEvent_t e : ctx->msm_events) (void)hipEventDestroy(e);
    verify_cache_release(ctx);
    delete ctx;
}

extern "C" int bpp_point_words(int curve_id) {
    switch (curve_id) {
        case BPP_BLS12_381_G1: return 2 * 6 + 1;
        case BPP_SECP256K1: return 2 * 4 + 1;
        case BPP_ED25519: return 2 * 4 + 1;
        default: return BPP_E_ARG;
    }
}

extern "C" int bpp_msm_batch(bpp_ctx* ctx, const uint64_t* scalars, const uint64_t* points, const uint32_t* lens,
                             size_t count, uint64_t* out) {
    if (!ctx || !out || (count && !lens)) return fail(BPP_E_ARG, "null argument");
    return on_ctx(*ctx, {count, "count"}, [&](auto cv) -> int {
        return MsmImpl<decltype(cv)>::msm_batch(scalars, points, lens, count, out);
    });
}

extern "C" int bpp_msm(bpp_ctx* ctx, const uint64_t* scalars, const uint64_t* points, size_t n, uint64_t* out) {
    return guarded({n, "n"}, [&] {
        const uint32_t len = (uint32_t)n;
        return bpp_msm_batch(ctx, scalars, points, &len, 1, out);
    });
}

extern "C" int bpp_msm_pippenger(bpp_ctx* ctx, const uint64_t* scalars, const uint64_t* points, size_t n,
                                 int window_bits, uint64_t* out) {
    if (!ctx || !out || (n && (!scalars || !points))) return fail(BPP_E_ARG, "null argument");
    return on_ctx(*ctx, [&](auto cv) -> int {
        return MsmImpl<decltype(cv)>::msm_pippenger(scalars, points, n, window_bits, out);
    });
}

extern "C" size_t bpp_msm_workspace_bytes(bpp_ctx* ctx, size_t n, int window_bits) {
    return size_for(ctx, [&](auto cv) { return MsmImpl<decltype(cv)>::msm_workspace_bytes(n, window_bits); });
}

extern "C" int bpp_msm_device(bpp_ctx* ctx, const uint64_t* d_scalars, const uint64_t* d_points, size_t n, int window_bits,
                              uint64_t* d_out, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!ctx || !d_out || !d_workspace || (n && (!d_scalars || !d_points))) return fail(BPP_E_ARG, "null argument");
    if (window_bits && (window_bits < 2 || window_bits > 16)) return fail(BPP_E_ARG, "window_bits must be in [2, 16]");
    return on_ctx(*ctx, [&](auto cv) -> int {
        return MsmImpl<decltype(cv)>::msm_device(reinterpret_cast<const uint32_t*>(d_scalars),
                                                 reinterpret_cast<const uint32_t*>(d_points), n, window_bits,
                                                 reinterpret_cast<uint32_t*>(d_out), d_status, d_workspace, workspace_bytes,
                                                 static_cast<hipStream_t>(stream), ctx);
    });
}

extern "C" int bpp_msm_set_profiling(bpp_ctx* ctx, int on) {
    if (!ctx) return fail(BPP_E_ARG, "null argument");
    return on_device(ctx->device, [&]() -> int {
        if (on && ctx->msm_events.empty()) {
            ctx->msm_events.resize(BPP_MSM_SLOTS * (PIP_STAGES + 1));
            for (hipEvent_t& e : ctx->msm_events) HIPCHK(hipEventCreate(&e));
        }
        ctx->msm_profiling = on != 0;
        ctx->msm_passes = 0;
        return BPP_OK;
    });
}

extern "C" int bpp_msm_profile(bpp_ctx* ctx, float* out_stage_ms, size_t* out_passes, uint32_t* out_shape) {
    if (!ctx || !out_stage_ms) return fail(BPP_E_ARG, "null argument");
    return on_device(ctx->device, [&]() -> int {
        const size_t np = std::min<size_t>(ctx->msm_passes, BPP_MSM_SLOTS);
        int rc = stage_means(ctx->msm_events.data(), np, PIP_STAGES + 1, PIP_STAGES, 1, out_stage_ms);
        if (rc) return rc;
        if (out_passes) *out_passes = np;
        if (out_shape) std::memcpy(out_shape, ctx->msm_shape, sizeof ctx->msm_shape);
        return BPP_OK;
    });
}

extern "C" int bpp_scalar_mul_batch(bpp_ctx* ctx, const uint64_t* scalars, const uint64_t* points, size_t n,
                                    uint64_t* out) {
    if (!ctx || !out || (n && (!scalars || !points))) return fail(BPP_E_ARG, "null argument");
    return on_ctx(*ctx, {n, "n"}, [&](auto cv) -> int {
        return MsmImpl<decltype(cv)>::scalar_mul_batch(scalars, points, n, out);
    });
}

extern "C" int bpp_pk_new(bpp_ctx* ctx, size_t length, uint64_t* out_gh, uint64_t* out_G, uint64_t* out_H) {
    if (!ctx || !out_gh || (length && (!out_G || !out_H))) return fail(BPP_E_ARG, "null argument");
    return on_ctx(*ctx, {length, "length"}, [&](auto cv) -> int {
        return MsmImpl<decltype(cv)>::pk_new(length, out_gh, out_G, out_H);
    });
}

extern "C" int bpp_pk_hashed(bpp_ctx* ctx, const uint8_t* label, size_t label_len, size_t length, uint64_t* out_gh,
                             uint64_t* out_G, uint64_t* out_H) {
    if (!ctx || !out_gh || (label_len && !label) || (length && (!out_G || !out_H))) return fail(BPP_E_ARG, "null argument");
    if (length > (1u << 24)) return fail(BPP_E_ARG, "length too large");
    return on_ctx(*ctx, [&](auto cv) -> int {
        return MsmImpl<decltype(cv)>::pk_hashed(label, label_len, length, out_gh, out_G, out_H);
    });
}

extern "C" int bpp_commit(bpp_ctx* ctx, const uint64_t* gh, uint64_t v, const uint64_t* gamma, uint64_t* out) {
    if (!ctx || !gh || !gamma || !out) return fail(BPP_E_ARG, "null argument");
    return on_ctx(*ctx, [&](auto cv) -> int { return MsmImpl<decltype(cv)>::commit(gh, v, gamma, out); });
}

extern "C" int bpp_range_verify(bpp_ctx* ctx, const uint64_t* gh, const uint64_t* G, const uint64_t* H, size_t n,
                                size_t m, const uint64_t* proof_points, size_t k, const uint64_t* proof_scalars,
                                const uint64_t* V) {
    if (!ctx || !gh || !G || !H || !proof_points || !proof_scalars || !V) return fail(BPP_E_ARG, "null argument");
    return on_ctx(*ctx, [&](auto cv) -> int {
        return literal_verify<decltype(cv)>(ctx, gh, G, H, n, m, proof_points, k, proof_scalars, V);
    });
}

extern "C" int bpp_set_verify_cache(bpp_ctx* ctx, int on) {
    if (!ctx) return fail(BPP_E_ARG, "null argument");
    return guarded([&] {
        ctx->verify_cache_off = on == 0;
        if (!on) verify_cache_release(ctx);
        return BPP_OK;
    });
}

extern "C" int bpp_range_prove(bpp_ctx* ctx, const uint64_t* gh, const uint64_t* G, const uint64_t* H, size_t n,
                               size_t m, const uint64_t* v, const uint64_t* gamma, const uint64_t* V,
                               uint64_t* out_points, uint64_t* out_scalars) {
    if (!ctx || !gh || !G || !H || !v || !gamma || !V || !out_points || !out_scalars)
        return fail(BPP_E_ARG, "null argument");
    return on_ctx(*ctx, {m, "m"}, [&](auto cv) -> int {
        return literal_prove<decltype(cv)>(ctx, gh, G, H, n, m, v, gamma, V, out_points, out_scalars);
    });
}

extern "C" int bpp_wip_fold_round(bpp_ctx* ctx, uint64_t* a, uint64_t* b, uint64_t* G, uint64_t* H, size_t len,
                                  const uint64_t* y_nhat, const uint64_t* e) {
    if (!ctx || !a || !b || !G || !H || !y_nhat || !e) return fail(BPP_E_ARG, "null argument");
    return on_ctx(*ctx, {len, "len"}, [&](auto cv) -> int {
        return ProveImpl<decltype(cv)>::wip_fold_round(a, b, G, H, len, y_nhat, e);
    });
}

// ---- batch verifier ------------------------------------------------------------------------------------
extern "C" int bpp_verifier_create(bpp_ctx* ctx, const uint64_t* gh, const uint64_t* G, const uint64_t* H, size_t n,
                                   size_t m, int window_bits, bpp_verifier** out) {
    if (!ctx || !gh || !G || !H || !out) return fail(BPP_E_ARG, "null argument");
    return on_ctx(*ctx, [&](auto cv) -> int {
        return VerifyImpl<decltype(cv)>::create(*ctx, gh, G, H, n, m, window_bits, out);
    });
}
extern "C" void bpp_verifier_destroy(bpp_verifier* v) { delete v; }

extern "C" size_t bpp_verifier_workspace_bytes(const bpp_verifier* v, size_t count) {
    return size_for(v, [&](auto cv) { return VerifyImpl<decltype(cv)>::ws_layout(v->s, count).total; });
}
extern "C" size_t bpp_verifier_msm_len(const bpp_verifier* v) { return v ? v->s.N : 0; }
extern "C" size_t bpp_verifier_table_bytes(const bpp_verifier* v) { return v ? v->table_bytes : 0; }
extern "C" const char* bpp_verifier_dominant_kernel(void) { return "k_fixed_msm"; }

extern "C" int bpp_verifier_run(bpp_verifier* v, const uint64_t* d_points, const uint64_t* d_scalars, size_t count,
                                const uint64_t* d_challenges, uint32_t* d_ok, void* d_workspace,
                                size_t workspace_bytes, uint64_t* d_out_scalars, uint64_t* d_out_result,
                                void* stream) {
    VerifyArgs a;
    a.points = d_points; a.scalars = d_scalars; a.count = count; a.challenges = d_challenges;
    a.ok = d_ok; a.out_scalars = d_out_scalars; a.out_result = d_out_result;
    if (int rc = verify_args(VERIFY_RUN, facts(v), 0, a, d_workspace)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int { return VerifyImpl<decltype(cv)>::run(v, a, d_workspace, workspace_bytes, hip(stream)); });
}

// ---- one pass as a HIP graph: captured once, replayed over the same buffers -----------------------------------
struct bpp_graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    int device = 0;
    ~bpp_graph() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
};
extern "C" void bpp_graph_destroy(bpp_graph* g) { delete g; }
extern "C" int bpp_verifier_graph_capture(bpp_verifier* v, const uint64_t* d_points, const uint64_t* d_scalars, size_t count,
                                          const uint64_t* d_challenges, uint32_t* d_ok, void* d_workspace,
                                          size_t workspace_bytes, bpp_graph** out) {
    VerifyArgs a;
    a.points = d_points; a.scalars = d_scalars; a.count = count; a.challenges = d_challenges; a.ok = d_ok;
    if (int rc = verify_args(VERIFY_GRAPH, facts(v), 0, a, out ? d_workspace : nullptr)) return rc;
    if (v->profiling) return fail(BPP_E_ARG, "switch the stage profiling off before capturing a pass");
    return on_ctx(v->ctx, [&](auto cv) -> int {
        hipStream_t cs = nullptr;
        HIPCHK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        const std::unique_ptr<std::remove_pointer_t<hipStream_t>, decltype(&hipStreamDestroy)> own_cs(cs, hipStreamDestroy);
        auto pass = [&] { return VerifyImpl<decltype(cv)>::run(v, a, d_workspace, workspace_bytes, cs); };
        // one eager pass first: it checks the arguments and creates what a pass creates lazily (the side stream and its
        // events of a lone batch), which must not happen inside a capture
        int rc = pass();
        if (rc) return rc;
        hipError_t e = hipStreamSynchronize(cs);
        if (e != hipSuccess) return fail(BPP_E_HIP, "eager pass before the capture failed: ", hipGetErrorString(e));
        auto g = std::make_unique<bpp_graph>();
        g->device = v->ctx.device;
        e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
        if (e == hipSuccess) {
            rc = guarded(pass);   // a pass that throws fails like one that returns an error
            const hipError_t e2 = hipStreamEndCapture(cs, &g->graph);   // always ends the capture, also after a failed pass
            if (rc) return rc;
            e = e2;
        }
        if (e == hipSuccess) e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
        if (e != hipSuccess) return fail(BPP_E_HIP, "graph capture failed: ", hipGetErrorString(e));
        *out = g.release();
        return BPP_OK;
    });
}
extern "C" int bpp_graph_launch(bpp_graph* g, void* stream) {
    if (!g || !g->exec) return fail(BPP_E_ARG, "null argument");
    return on_device(g->device, [&]() -> int {
        HIPCHK(hipGraphLaunch(g->exec, static_cast<hipStream_t>(stream)));
        return BPP_OK;
    });
}

// ---- the prover entries: the batched range prover (impl_prove_batch.hpp), here and under "proving blocks of mixed
// aggregation sizes", and the seam's (impl_wip.hpp).  Each fills its record and passes prove_args ------------------------
namespace {
// the argument checks the four seam entries share; 0: go on
int wip_args(size_t nv, int flags, bool have_transcript) {
    if (nv > VS_MAXM) return fail(BPP_E_ARG, "nv exceeds the supported maximum (64)");
    if (flags & ~BPP_SER_TRANSCRIPT) return fail(BPP_E_ARG, "unknown flag");
    if ((flags & BPP_SER_TRANSCRIPT) && !have_transcript) return fail(BPP_E_ARG, "BPP_SER_TRANSCRIPT needs the transcript states");
    return BPP_OK;
}

// What tells the prover entries' checks apart; the checks, their order and every other text are prove_args.
struct ProveEntry {
    int flags;          // the flags it takes (an entry without a flags argument says what its name says)
    bool empty_first;   // a count of zero is answered ahead of the buffers, the blinding and the count (the mixed entries)
    const char* both;   // what a blind_key beside blinding scalars is told; null: the blinding is not looked at here
    bool one_launch;    // the count is bounded here (the mixed host forms: behind their plan likewise)
};
constexpr int PROVE_MIXED_FLAGS = BPP_SER_TRANSCRIPT | BPP_PROVE_AMOUNT64, PROVE_SER_FLAGS = PROVE_MIXED_FLAGS | BPP_SER_UNCOMPRESSED;
constexpr const char* BOTH_MIXED = "blind_key and d_blinding are both given";
constexpr ProveEntry PROVE_FIXED{BPP_SER_TRANSCRIPT, false, nullptr, false};
constexpr ProveEntry PROVE_MIXED_DEVICE{PROVE_MIXED_FLAGS, true, BOTH_MIXED, true}, PROVE_MIXED_HOST{PROVE_MIXED_FLAGS, true, nullptr, false};
constexpr ProveEntry PROVE_SER_DEVICE{PROVE_SER_FLAGS, true, BOTH_MIXED, true}, PROVE_SER_HOST{PROVE_SER_FLAGS, true, nullptr, false};
constexpr ProveEntry PROVE_SEAM{BPP_SER_TRANSCRIPT, false, "give blind_key or d_blinding, not both", false};

// the one decoding of an entry's flags into its record, behind the refusal of those it does not take
int prove_flags(const ProveEntry& e, int flags, ProveArgs& a) noexcept {
    if (flags & ~e.flags) return fail(BPP_E_ARG, "unknown flag");
    a.fs = (flags & BPP_SER_TRANSCRIPT) != 0;
    a.amount64 = (flags & BPP_PROVE_AMOUNT64) != 0;
    a.version = (flags & BPP_SER_UNCOMPRESSED) ? 2u : 1u;
    return BPP_OK;
}
int prove_flags(const ProveEntry&, int flags, WipProveArgs& a) noexcept {
    if (int rc = wip_args(a.nv, flags, a.transcript != nullptr)) return rc;
    a.fs = (flags & BPP_SER_TRANSCRIPT) != 0;
    return BPP_OK;
}

// The checks of the ten prover entries.  a holds the entry's pointers and leaves with what the flags say; buffers: whether
// every buffer that a count above zero reads or writes, the optional ones aside, is there (a device entry: the workspace
// too).  A count of zero passes and is answered by the entry.
template <class A>
int prove_args(const bpp_verifier* engine, const ProveEntry& e, int flags, A& a, bool buffers) noexcept {
    if (!engine || (!e.empty_first && !buffers)) return fail(BPP_E_ARG, "null argument");
    if (int rc = prove_flags(e, flags, a)) return rc;
    if (e.empty_first) {
        if (a.count == 0) return BPP_OK;
        if (!buffers) return fail(BPP_E_ARG, "null argument");
    }
    if (e.both) {
        if (a.blind_key && a.blinding) return fail(BPP_E_ARG, e.both);
        if ((a.blind_key || a.blinding) && !a.fs) return fail(BPP_E_ARG, "blinding needs BPP_SER_TRANSCRIPT");
    }
    if (e.one_launch && a.count > 0x7fffffffu / 64) return fail(BPP_E_ARG, "count too large for one launch");
    return BPP_OK;
}
}  // namespace

extern "C" int bpp_range_prove_batch(bpp_verifier* engine, const uint64_t* v, const uint64_t* gamma, size_t count,
                                     uint64_t* out_points, uint64_t* out_scalars, uint64_t* out_V) {
    ProveArgs a;
    a.values = v; a.gammas = gamma; a.count = count;
    a.out_points = out_points; a.out_scalars = out_scalars; a.out_V = out_V;
    if (int rc = prove_args(engine, PROVE_FIXED, 0, a, v && gamma && out_points && out_scalars)) return rc;
    if (count == 0) return BPP_OK;
    return on_ctx(engine->ctx, {count, "count"}, [&](auto cv) -> int { return ProveBatchImpl<decltype(cv)>::prove_host(engine, a); });
}

extern "C" int bpp_range_prove_batch_fs(bpp_verifier* engine, const uint64_t* v, const uint64_t* gamma, size_t count,
                                        const uint8_t* blind_key, uint64_t index_base, uint64_t* out_points,
                                        uint64_t* out_scalars, uint64_t* out_V) {
    ProveArgs a;
    a.values = v; a.gammas = gamma; a.count = count; a.blind_key = blind_key; a.index_base = index_base;
    a.out_points = out_points; a.out_scalars = out_scalars; a.out_V = out_V;
    if (int rc = prove_args(engine, PROVE_FIXED, BPP_SER_TRANSCRIPT, a, v && gamma && out_points && out_scalars)) return rc;
    if (count == 0) return BPP_OK;
    return on_ctx(engine->ctx, {count, "count"}, [&](auto cv) -> int { return ProveBatchImpl<decltype(cv)>::prove_host(engine, a); });
}

extern "C" size_t bpp_prover_workspace_bytes(const bpp_verifier* engine, size_t count) {
    return size_for(engine, [&](auto cv) { return ProveBatchImpl<decltype(cv)>::prove_layout(engine->s, count).total; });
}

extern "C" int bpp_range_prove_batch_device(bpp_verifier* engine, const uint64_t* d_v, const uint64_t* d_gamma,
                                            size_t count, uint64_t* d_out_points, uint64_t* d_out_scalars,
                                            uint64_t* d_out_V, void* d_workspace, size_t workspace_bytes, void* stream) {
    ProveArgs a;
    a.values = d_v; a.gammas = d_gamma; a.count = count;
    a.out_points = d_out_points; a.out_scalars = d_out_scalars; a.out_V = d_out_V;
    if (int rc = prove_args(engine, PROVE_FIXED, 0, a, d_v && d_gamma && d_out_points && d_out_scalars && d_workspace)) return rc;
    if (count == 0) return BPP_OK;
    return on_ctx(engine->ctx, {count, "count"}, [&](auto cv) -> int {
        return ProveBatchImpl<decltype(cv)>::prove_device(engine, a, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream));
    });
}

// blind_key beside d_blinding is taken here: the buffer wins
extern "C" int bpp_range_prove_batch_fs_device(bpp_verifier* engine, const uint64_t* d_v, const uint64_t* d_gamma,
                                               size_t count, const uint8_t* blind_key, uint64_t index_base,
                                               const uint64_t* d_blinding, uint64_t* d_out_points, uint64_t* d_out_scalars,
                                               uint64_t* d_out_V, uint64_t* d_out_challenges, void* d_workspace,
                                               size_t workspace_bytes, void* stream) {
    ProveArgs a;
    a.values = d_v; a.gammas = d_gamma; a.count = count;
    a.blind_key = blind_key; a.index_base = index_base; a.blinding = d_blinding;
    a.out_points = d_out_points; a.out_scalars = d_out_scalars; a.out_V = d_out_V; a.out_challenges = d_out_challenges;
    if (int rc = prove_args(engine, PROVE_FIXED, BPP_SER_TRANSCRIPT, a, d_v && d_gamma && d_out_points && d_out_scalars && d_workspace))
        return rc;
    if (count == 0) return BPP_OK;
    return on_ctx(engine->ctx, {count, "count"}, [&](auto cv) -> int {
        return ProveBatchImpl<decltype(cv)>::prove_device(engine, a, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream));
    });
}

// ---- the WIP seam (impl_wip.hpp) -------------------------------------------------------------------------
extern "C" size_t bpp_wip_prover_workspace_bytes(const bpp_verifier* engine, size_t count) {
    if (count >> 32) return 0;
    return size_for(engine, [&](auto cv) { return WipImpl<decltype(cv)>::prove_ws(engine, count).total; });
}
extern "C" size_t bpp_wip_verifier_workspace_bytes(const bpp_verifier* v, size_t count, size_t nv) {
    if (nv > VS_MAXM || count > 0x7fffffffu / 64) return 0;
    return size_for(v, [&](auto cv) { return WipImpl<decltype(cv)>::verify_ws(v, count, nv).total; });
}
extern "C" int bpp_wip_prove_batch_device(bpp_verifier* engine, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_y,
                                          const uint64_t* d_gamma, size_t count, size_t nv, int flags, const void* d_transcript,
                                          const uint8_t* blind_key, uint64_t index_base, const uint64_t* d_blinding,
                                          uint64_t* d_out_points, uint64_t* d_out_scalars, uint64_t* d_out_challenges,
                                          void* d_workspace, size_t workspace_bytes, void* stream) {
    WipProveArgs a{d_a, d_b, d_y, d_gamma, count, nv};
    a.transcript = d_transcript;
    a.blind_key = blind_key; a.index_base = index_base; a.blinding = d_blinding;
    a.points = d_out_points; a.out_scalars = d_out_scalars; a.out_challenges = d_out_challenges;
    if (int rc = prove_args(engine, PROVE_SEAM, flags, a, d_a && d_b && d_y && d_gamma && d_out_points && d_out_scalars && d_workspace))
        return rc;
    if (count == 0) return BPP_OK;
    return on_ctx(engine->ctx, {count, "count"}, [&](auto cv) -> int {
        return WipImpl<decltype(cv)>::prove_device(engine, a, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream));
    });
}
extern "C" int bpp_wip_verify_batch_device(bpp_verifier* v, const uint64_t* d_points, const uint64_t* d_scalars,
                                           const uint64_t* d_y, const uint64_t* d_statement, size_t nv, size_t count, int flags,
                                           const void* d_transcript, const uint64_t* d_challenges, uint32_t* d_ok,
                                           void* d_workspace, size_t workspace_bytes, uint64_t* d_out_scalars,
                                           uint64_t* d_out_result, void* stream) {
    if (!v || !d_points || !d_scalars || !d_y || !d_statement || !d_ok || !d_workspace) return fail(BPP_E_ARG, "null argument");
    const int rc = wip_args(nv, flags, d_transcript || d_challenges);   // explicit challenges need no transcript
    if (rc) return rc;
    if (count == 0) return BPP_OK;
    if (count > 0x7fffffffu / 64) return fail(BPP_E_ARG, "count too large for one launch");
    return on_ctx(v->ctx, [&](auto cv) -> int {
        return WipImpl<decltype(cv)>::verify_device(v, d_points, d_scalars, d_y, d_statement, nv, count,
                                                    (flags & BPP_SER_TRANSCRIPT) != 0, d_transcript, d_challenges, d_ok,
                                                    d_workspace, workspace_bytes, d_out_scalars, d_out_result,
                                                    static_cast<hipStream_t>(stream));
    });
}
extern "C" int bpp_wip_prove_batch(bpp_verifier* engine, const uint64_t* a, const uint64_t* b, const uint64_t* y,
                                   const uint64_t* gamma, size_t count, size_t nv, int flags, const void* transcript,
                                   const uint8_t* blind_key, uint64_t index_base, const uint64_t* blinding, uint64_t* points,
                                   uint64_t* out_scalars, uint64_t* out_challenges) {
    WipProveArgs w{a, b, y, gamma, count, nv};
    w.transcript = transcript;
    w.blind_key = blind_key; w.index_base = index_base; w.blinding = blinding;
    w.points = points; w.out_scalars = out_scalars; w.out_challenges = out_challenges;
    if (int rc = prove_args(engine, PROVE_SEAM, flags, w, a && b && y && gamma && points && out_scalars)) return rc;
    if (count == 0) return BPP_OK;
    return on_ctx(engine->ctx, {count, "count"}, [&](auto cv) -> int { return WipImpl<decltype(cv)>::prove_host(engine, w); });
}
extern "C" int bpp_wip_verify_batch(bpp_verifier* v, const uint64_t* points, const uint64_t* scalars, const uint64_t* y,
                                    const uint64_t* statement, size_t nv, size_t count, int flags, const void* transcript,
                                    const uint64_t* challenges, uint32_t* out_ok, uint64_t* out_scalars,
                                    uint64_t* out_result) {
    if (!v || !points || !scalars || !y || !statement || !out_ok) return fail(BPP_E_ARG, "null argument");
    const int rc = wip_args(nv, flags, transcript || challenges);
    if (rc) return rc;
    if (count == 0) return BPP_OK;
    if (count > 0x7fffffffu / 64) return fail(BPP_E_ARG, "count too large for one launch");
    return on_ctx(v->ctx, [&](auto cv) -> int {
        const bool fs = (flags & BPP_SER_TRANSCRIPT) != 0 && !challenges;
        return WipImpl<decltype(cv)>::verify_host(v, points, scalars, y, statement, nv, count, fs, fs ? transcript : nullptr,
                                                  challenges, out_ok, out_scalars, out_result);
    });
}

// ---- combined batch check ------------------------------------------------------------------------------
extern "C" size_t bpp_verifier_partial_bytes(const bpp_verifier* v) {
    return size_for(v, [&](auto cv) { return (size_t)partial_words<decltype(cv)>() * 4; });
}
extern "C" size_t bpp_verifier_combined_workspace_bytes(const bpp_verifier* v, size_t count) {
    return size_for(v, [&](auto cv) { return VerifyImpl<decltype(cv)>::comb_layout(v->s, count).total; });
}
extern "C" int bpp_verifier_run_combined(bpp_verifier* v, const uint64_t* d_points, const uint64_t* d_scalars,
                                         size_t count, const uint64_t* d_challenges, const uint8_t* weight_key,
                                         uint64_t index_base, const uint64_t* d_weights, void* d_out_partial,
                                         uint32_t* d_ok, void* d_workspace, size_t workspace_bytes, void* stream) {
    VerifyArgs a;
    a.points = d_points; a.scalars = d_scalars; a.count = count; a.challenges = d_challenges;
    a.weight_key = weight_key; a.index_base = index_base; a.weights = d_weights;
    a.ok = d_ok; a.out_partial = static_cast<uint32_t*>(d_out_partial);
    if (int rc = verify_args(VERIFY_COMBINED, facts(v), 0, a, d_workspace)) return rc;
    return on_ctx(v->ctx, [&](auto cv) -> int { return VerifyImpl<decltype(cv)>::run_combined(v, a, d_workspace, workspace_bytes, hip(stream)); });
}
// ---- grouped check: per-proof verdicts, one weighted check per group, exact pass over the failing groups ------
extern "C" size_t bpp_verifier_grouped_workspace_bytes(const bpp_verifier* v, size_t count, uint32_t group) {
    if (!group_ok(group)) return 0;
    return size_for(v, [&](auto cv) { return VerifyImpl<decltype(cv)>::group_layout(v->s, count, group).total; });
}
extern "C" int bpp_verifier_run_grouped(bpp_verifier* v, const uint64_t* d_points, const uint64_t* d_scalars, size_t count,
                                        const uint64_t* d_challenges, const uint8_t* weight_key, uint64_t index_base,
                                        const uint64_t* d_weights, uint32_t group, uint32_t* d_out_verdicts,
                                        uint64_t* stats, void* d_workspace, size_t workspace_bytes, void* stream) {
    VerifyArgs a;
    a.points = d_points; a.scalars = d_scalars; a.count = count; a.challenges = d_challenges;
    a.weight_key = weight_key; a.index_base = index_base; a.weights = d_weights; a.group = group;
    a.ok = d_out_verdicts; a.stats = stats;
    if (int rc = verify_args(VERIFY_GROUPED, facts(v), 0, a, d_workspace)) return rc;
    return on_ctx(v->ctx, [&](auto cv) -> int { return VerifyImpl<decltype(cv)>::run_grouped(v, a, d_workspace, workspace_bytes, hip(stream)); });
}
// the grouped check in two calls (one host thread, several batches in flight)
extern "C" int bpp_verifier_grouped_begin(bpp_verifier* v, const uint64_t* d_points, const uint64_t* d_scalars, size_t count,
                                          const uint64_t* d_challenges, const uint8_t* weight_key, uint64_t index_base,
                                          const uint64_t* d_weights, uint32_t group, uint32_t* d_out_verdicts,
                                          void* d_workspace, size_t workspace_bytes, void* stream) {
    VerifyArgs a;
    a.points = d_points; a.scalars = d_scalars; a.count = count; a.challenges = d_challenges;
    a.weight_key = weight_key; a.index_base = index_base; a.weights = d_weights; a.group = group;
    a.ok = d_out_verdicts;
    if (int rc = verify_args(VERIFY_GROUPED, facts(v), 0, a, d_workspace)) return rc;
    return on_ctx(v->ctx, [&](auto cv) -> int { return VerifyImpl<decltype(cv)>::grouped_begin(v, a, d_workspace, workspace_bytes, hip(stream)); });
}
extern "C" int bpp_verifier_grouped_finish(bpp_verifier* v, const uint64_t* d_points, const uint64_t* d_scalars, size_t count,
                                           const uint64_t* d_challenges, uint32_t group, uint32_t* d_out_verdicts,
                                           uint64_t* stats, void* d_workspace, size_t workspace_bytes, void* stream) {
    VerifyArgs a;
    a.points = d_points; a.scalars = d_scalars; a.count = count; a.challenges = d_challenges;
    a.group = group; a.ok = d_out_verdicts; a.stats = stats;
    if (int rc = verify_args(VERIFY_GROUPED_FINISH, facts(v), 0, a, d_workspace)) return rc;
    return on_ctx(v->ctx, [&](auto cv) -> int {
        return VerifyImpl<decltype(cv)>::grouped_finish(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}
extern "C" int bpp_verifier_sum_partials(bpp_verifier* v, const void* d_partials, size_t n, uint32_t* d_ok,
                                         void* stream) {
    if (!v || !d_partials || !d_ok) return fail(BPP_E_ARG, "null argument");
    return on_ctx(v->ctx, {n, "n"}, [&](auto cv) -> int {
        return VerifyImpl<decltype(cv)>::sum_partials(static_cast<const uint32_t*>(d_partials), n, d_ok,
                                                      static_cast<hipStream_t>(stream));
    });
}

extern "C" int bpp_verifier_derive_challenges(bpp_verifier* v, const uint64_t* d_points, size_t count,
                                              uint64_t* d_challenges, void* stream) {
    VerifyArgs a;
    a.points = d_points; a.count = count; a.out_challenges = d_challenges;
    if (int rc = verify_args(VERIFY_DERIVE, facts(v), 0, a, nullptr)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int { return VerifyImpl<decltype(cv)>::derive_challenges(v, a, nullptr, 0, hip(stream)); });
}

extern "C" int bpp_verifier_set_subgroup_check(bpp_verifier* v, int on) {
    if (!v) return fail(BPP_E_ARG, "null argument");
    v->check_subgroup = on != 0;
    return BPP_OK;
}

extern "C" int bpp_verifier_set_profiling(bpp_verifier* v, int on) {
    if (!v) return fail(BPP_E_ARG, "null argument");
    return on_device(v->ctx.device, [&]() -> int {
        if (on && v->events.empty()) {
            v->events.resize((size_t)BPP_PROFILE_SLOTS * BPP_NUM_STAGES * 2);
            for (hipEvent_t& e : v->events) HIPCHK(hipEventCreate(&e));
        }
        v->profiling = on != 0;
        v->passes_recorded = 0;
        return BPP_OK;
    });
}

extern "C" int bpp_verifier_profile(bpp_verifier* v, float* out_stage_ms, size_t* out_passes,
                                    unsigned* out_blocks_per_proof) {
    if (!v || !out_stage_ms) return fail(BPP_E_ARG, "null argument");
    return on_device(v->ctx.device, [&]() -> int {
        const size_t np = std::min<size_t>(v->passes_recorded, BPP_PROFILE_SLOTS);
        int rc = stage_means(v->events.data(), np, BPP_NUM_STAGES * 2, BPP_NUM_STAGES, 2, out_stage_ms);
        if (rc) return rc;
        if (out_passes) *out_passes = np;
        if (out_blocks_per_proof) *out_blocks_per_proof = v->last_blocks_per_proof;
        return BPP_OK;
    });
}

extern "C" int bpp_range_verify_batch(bpp_verifier* v, const uint64_t* points, const uint64_t* scalars, size_t count,
                                      uint32_t* out_ok) {
    VerifyArgs a;
    a.points = points; a.scalars = scalars; a.count = count; a.ok = out_ok;
    if (int rc = verify_args(VERIFY_HOST, facts(v), 0, a, nullptr)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int { return VerifyImpl<decltype(cv)>::verify_host(v, a, HOST_WIRE, 0); });
}

// ---- mixed batches: proof i of shape (n, m_i) against the verifier's (n, m) tables (mixed.hpp) ------------------
extern "C" size_t bpp_verifier_mixed_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count) {
    if (count && !m_of) return 0;
    return size_for(v, [&](auto cv) { return VerifyImpl<decltype(cv)>::mixed_workspace_bytes(v, m_of, count); });
}

extern "C" int bpp_verifier_run_mixed(bpp_verifier* v, const uint64_t* d_points, const uint64_t* d_scalars,
                                      const uint32_t* m_of, size_t count, const uint64_t* d_challenges, uint32_t* d_ok,
                                      void* d_workspace, size_t workspace_bytes, uint64_t* d_out_result, void* stream) {
    VerifyArgs a;
    a.points = d_points; a.scalars = d_scalars; a.m_of = m_of; a.count = count; a.challenges = d_challenges;
    a.ok = d_ok; a.out_result = d_out_result;
    if (int rc = verify_args(VERIFY_MIXED, facts(v), 0, a, d_workspace)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int { return VerifyImpl<decltype(cv)>::run_mixed(v, a, d_workspace, workspace_bytes, hip(stream)); });
}

extern "C" int bpp_verifier_derive_challenges_mixed(bpp_verifier* v, const uint64_t* d_points, const uint32_t* m_of,
                                                    size_t count, uint64_t* d_challenges, void* d_workspace,
                                                    size_t workspace_bytes, void* stream) {
    VerifyArgs a;
    a.points = d_points; a.m_of = m_of; a.count = count; a.out_challenges = d_challenges;
    if (int rc = verify_args(VERIFY_DERIVE_MIXED, facts(v), 0, a, d_workspace)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int {
        return VerifyImpl<decltype(cv)>::derive_challenges_mixed(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

extern "C" int bpp_range_verify_batch_mixed(bpp_verifier* v, const uint64_t* points, const uint64_t* scalars,
                                            const uint32_t* m_of, size_t count, uint32_t* out_ok) {
    VerifyArgs a;
    a.points = points; a.scalars = scalars; a.m_of = m_of; a.count = count; a.ok = out_ok;
    if (int rc = verify_args(VERIFY_HOST_MIXED, facts(v), 0, a, nullptr)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int { return VerifyImpl<decltype(cv)>::verify_host(v, a, HOST_MIXED, 0); });
}

// ---- compressed point encodings (codec.hpp) ---------------------------------------------------------------
extern "C" size_t bpp_point_compressed_bytes(int curve_id) {
    switch (curve_id) {
        case BPP_BLS12_381_G1: return 48;
        case BPP_SECP256K1: return 33;
        case BPP_ED25519: return 32;   /* ristretto255 */
        default: return 0;
    }
}

extern "C" int bpp_points_compress(bpp_ctx* ctx, const uint64_t* points, size_t n, uint8_t* out) {
    if (!ctx || (n && (!points || !out))) return fail(BPP_E_ARG, "null argument");
    return on_ctx(*ctx, {n, "n"}, [&](auto cv) -> int { return CodecImpl<decltype(cv)>::compress(points, n, out); });
}

extern "C" int bpp_points_decompress(bpp_ctx* ctx, const uint8_t* in, size_t n, uint64_t* out_points, uint32_t* out_ok) {
    if (!ctx || (n && (!in || !out_points || !out_ok))) return fail(BPP_E_ARG, "null argument");
    return on_ctx(*ctx, {n, "n"}, [&](auto cv) -> int { return CodecImpl<decltype(cv)>::decompress(in, n, out_points, out_ok); });
}

extern "C" int bpp_points_decompress_device(bpp_ctx* ctx, const void* d_in, size_t n, uint64_t* d_points, uint32_t* d_ok,
                                            int check_subgroup, void* stream) {
    if (!ctx || (n && (!d_in || !d_points || !d_ok))) return fail(BPP_E_ARG, "null argument");
    return on_ctx(*ctx, {n, "n"}, [&](auto cv) -> int {
        return CodecImpl<decltype(cv)>::decompress_device(static_cast<const uint8_t*>(d_in), n, d_points, d_ok,
                                                          static_cast<hipStream_t>(stream), check_subgroup != 0);
    });
}

extern "C" int bpp_range_verify_batch_compressed(bpp_verifier* v, const uint8_t* records, const uint64_t* scalars,
                                                 size_t count, uint32_t* out_ok) {
    VerifyArgs a;
    a.proofs = records; a.scalars = scalars; a.count = count; a.ok = out_ok;
    if (int rc = verify_args(VERIFY_HOST_COMPRESSED, facts(v), 0, a, nullptr)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int { return VerifyImpl<decltype(cv)>::verify_host(v, a, HOST_COMPRESSED, 0); });
}

// ---- serialized proofs (the container; see include/bpp_amd.h) -----------------------------------------------------
extern "C" size_t bpp_point_uncompressed_bytes(int curve_id) {
    switch (curve_id) {
        case BPP_BLS12_381_G1: return 96;
        case BPP_SECP256K1: return 65;
        default: return 0;   /* ristretto255 has no uncompressed form */
    }
}
static size_t container_point_size(int curve_id, int version) {
    return version == 2 ? bpp_point_uncompressed_bytes(curve_id) : (version == 1 ? bpp_point_compressed_bytes(curve_id) : 0);
}
extern "C" size_t bpp_proof_bytes_version(int curve_id, size_t n, size_t m, int version) {
    const size_t cb = container_point_size(curve_id, version);
    const size_t mn = n * m;
    if (cb == 0 || mn == 0 || (mn & (mn - 1))) return 0;
    return CONTAINER_HDR + (3 + 2 * (size_t)log2_exact(mn)) * cb + 96;
}
extern "C" size_t bpp_proof_bytes(int curve_id, size_t n, size_t m) { return bpp_proof_bytes_version(curve_id, n, m, 1); }

extern "C" int bpp_points_uncompressed(bpp_ctx* ctx, const uint64_t* points, size_t n, uint8_t* out) {
    if (!ctx || (n && (!points || !out))) return fail(BPP_E_ARG, "null argument");
    if (bpp_point_uncompressed_bytes(ctx->curve) == 0) return fail(BPP_E_ARG, "no uncompressed form for this curve");
    return guarded({n, "n"}, [&] {
        points_to_uncompressed(ctx->curve, points, n, out);
        return BPP_OK;
    });
}

extern "C" int bpp_proofs_encode_version(bpp_ctx* ctx, size_t n, size_t m, int version, const uint64_t* points,
                                         const uint64_t* scalars, size_t count, uint8_t* out) {
    if (!ctx || (count && (!points || !scalars || !out))) return fail(BPP_E_ARG, "null argument");
    const size_t pb = bpp_proof_bytes_version(ctx->curve, n, m, version);
    if (pb == 0 || n > 255 || m > 255) return fail(BPP_E_ARG, "n*m must be a power of two (n, m <= 255); version 1 or 2");
    if (count == 0) return BPP_OK;
    return on_ctx(*ctx, {count, "count"}, [&](auto cv) -> int {
        return CodecImpl<decltype(cv)>::encode_host(n, m, version, points, scalars, count, out);
    });
}

extern "C" int bpp_proofs_encode(bpp_ctx* ctx, size_t n, size_t m, const uint64_t* points, const uint64_t* scalars,
                                 size_t count, uint8_t* out) {
    return bpp_proofs_encode_version(ctx, n, m, 1, points, scalars, count, out);
}

extern "C" int bpp_proofs_decode(bpp_ctx* ctx, size_t n, size_t m, const uint8_t* in, size_t count, uint64_t* out_points,
                                 uint64_t* out_scalars, uint32_t* out_status) {
    if (!ctx || (count && (!in || !out_points || !out_scalars || !out_status))) return fail(BPP_E_ARG, "null argument");
    if (count == 0) return BPP_OK;
    const size_t pb = bpp_proof_bytes(ctx->curve, n, m);
    if (pb == 0 || n > 255 || m > 255) return fail(BPP_E_ARG, "n*m must be a power of two (n, m <= 255)");
    return on_ctx(*ctx, {count, "count"}, [&](auto cv) -> int {
        return CodecImpl<decltype(cv)>::decode_host(n, m, in, count, out_points, out_scalars, out_status);
    });
}

extern "C" size_t bpp_verifier_serialized_workspace_bytes(const bpp_verifier* v, size_t count) {
    return size_for(v, [&](auto cv) { return VerifyImpl<decltype(cv)>::ser_layout(v->s, count).total; });
}

extern "C" int bpp_range_verify_batch_serialized_device(bpp_verifier* v, const void* d_proofs, const void* d_commitments,
                                                        size_t count, int flags, uint32_t* d_ok, void* d_workspace,
                                                        size_t workspace_bytes, void* stream) {
    VerifyArgs a;
    a.proofs = static_cast<const uint8_t*>(d_proofs); a.commitments = static_cast<const uint8_t*>(d_commitments);
    a.count = count; a.ok = d_ok;
    if (int rc = verify_args(VERIFY_SER, facts(v), flags, a, d_workspace)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int {
        return VerifyImpl<decltype(cv)>::run_serialized(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

// the same with the grouped check behind the decoder (per-proof statuses; synchronises the stream)
extern "C" size_t bpp_verifier_serialized_grouped_workspace_bytes(const bpp_verifier* v, size_t count, uint32_t group) {
    if (!group_ok(group)) return 0;
    return size_for(v, [&](auto cv) { return VerifyImpl<decltype(cv)>::ser_layout(v->s, count, group).total; });
}
extern "C" int bpp_range_verify_batch_serialized_grouped_device(bpp_verifier* v, const void* d_proofs, const void* d_commitments,
                                                                size_t count, int flags, const uint8_t* weight_key,
                                                                uint64_t index_base, uint32_t group, uint32_t* d_ok,
                                                                uint64_t* stats, void* d_workspace, size_t workspace_bytes,
                                                                void* stream) {
    VerifyArgs a;
    a.proofs = static_cast<const uint8_t*>(d_proofs); a.commitments = static_cast<const uint8_t*>(d_commitments);
    a.count = count; a.weight_key = weight_key; a.index_base = index_base; a.group = group; a.ok = d_ok; a.stats = stats;
    if (int rc = verify_args(VERIFY_SER_GROUPED, facts(v), flags, a, d_workspace)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int {
        return VerifyImpl<decltype(cv)>::run_serialized(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

// host buffers in, host verdicts out: the device path above between two copies
extern "C" int bpp_range_verify_batch_serialized(bpp_verifier* v, const uint8_t* proofs, const uint8_t* commitments,
                                                 size_t count, int flags, uint32_t* out_ok) {
    VerifyArgs a;
    a.proofs = proofs; a.commitments = commitments; a.count = count; a.ok = out_ok;
    if (int rc = verify_args(VERIFY_HOST_SER, facts(v), flags, a, nullptr)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int { return VerifyImpl<decltype(cv)>::verify_host(v, a, HOST_SERIALIZED, flags); });
}

// ---- serialized proofs of mixed aggregation sizes (mixed.hpp; the framing of a bare stream: container_scan.hpp) ----
extern "C" int bpp_proofs_scan(int curve_id, size_t n, int version, const uint8_t* proofs, size_t proofs_bytes,
                               uint32_t* m_of, size_t max_count, size_t* out_count) {
    if (!out_count || (proofs_bytes && !proofs) || (max_count && !m_of)) return fail(BPP_E_ARG, "null argument");
    *out_count = 0;
    return guarded({max_count, "max_count"}, [&]() -> int {
        const ScanResult r = container_scan(curve_id, n, version, proofs, proofs_bytes, m_of, max_count);
        *out_count = r.count;
        if (r.status == SCAN_OK) return BPP_OK;
        if (r.status == SCAN_BAD_ARG) return fail(BPP_E_ARG, "bpp_proofs_scan: ", scan_status_text(r.status));
        return fail(r.status == SCAN_TOO_MANY ? BPP_E_ARG : BPP_E_LENGTH,
                    "container " + std::to_string(r.count) + " at byte " + std::to_string(r.offset) + ": " +
                        scan_status_text(r.status));
    });
}

extern "C" size_t bpp_verifier_serialized_mixed_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count) {
    if (!mixed_sizes_ok(m_of, count)) return 0;
    return size_for(v, [&](auto cv) { return VerifyImpl<decltype(cv)>::ser_mixed_workspace_bytes(v, m_of, count); });
}

extern "C" int bpp_range_verify_batch_serialized_mixed_device(bpp_verifier* v, const void* d_proofs, const void* d_commitments,
                                                              const uint32_t* m_of, size_t count, int flags, uint32_t* d_ok,
                                                              void* d_workspace, size_t workspace_bytes, void* stream) {
    VerifyArgs a;
    a.proofs = static_cast<const uint8_t*>(d_proofs); a.commitments = static_cast<const uint8_t*>(d_commitments);
    a.m_of = m_of; a.count = count; a.ok = d_ok;
    if (int rc = verify_args(VERIFY_SER_MIXED, facts(v), flags, a, d_workspace)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int {
        return VerifyImpl<decltype(cv)>::run_serialized_mixed(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

// host buffers in, host verdicts out: the device path above between two copies
extern "C" int bpp_range_verify_batch_serialized_mixed(bpp_verifier* v, const uint8_t* proofs, const uint8_t* commitments,
                                                       const uint32_t* m_of, size_t count, int flags, uint32_t* out_ok) {
    VerifyArgs a;
    a.proofs = proofs; a.commitments = commitments; a.m_of = m_of; a.count = count; a.ok = out_ok;
    if (int rc = verify_args(VERIFY_HOST_SER_MIXED, facts(v), flags, a, nullptr)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int { return VerifyImpl<decltype(cv)>::verify_host(v, a, HOST_SERIALIZED_MIXED, flags); });
}

// ---- the grouped check over mixed batches, wire records and bytes (impl_verify.hpp "grouped check over a MIXED batch") ----
extern "C" size_t bpp_verifier_grouped_mixed_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count,
                                                             uint32_t group) {
    if (!mixed_sizes_ok(m_of, count)) return 0;
    return size_for(v, [&](auto cv) { return VerifyImpl<decltype(cv)>::grouped_mixed_workspace_bytes(v, m_of, count, group); });
}

extern "C" int bpp_verifier_run_grouped_mixed(bpp_verifier* v, const uint64_t* d_points, const uint64_t* d_scalars,
                                              const uint32_t* m_of, size_t count, const uint64_t* d_challenges,
                                              const uint8_t* weight_key, uint64_t index_base, const uint64_t* d_weights,
                                              uint32_t group, uint32_t* d_out_verdicts, uint64_t* stats, void* d_workspace,
                                              size_t workspace_bytes, void* stream) {
    VerifyArgs a;
    a.points = d_points; a.scalars = d_scalars; a.m_of = m_of; a.count = count; a.challenges = d_challenges;
    a.weight_key = weight_key; a.index_base = index_base; a.weights = d_weights; a.group = group;
    a.ok = d_out_verdicts; a.stats = stats;
    if (int rc = verify_args(VERIFY_GROUPED_MIXED, facts(v), 0, a, d_workspace)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int {
        return VerifyImpl<decltype(cv)>::run_grouped_mixed(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

extern "C" size_t bpp_verifier_serialized_grouped_mixed_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of,
                                                                        size_t count, uint32_t group) {
    if (!mixed_sizes_ok(m_of, count)) return 0;
    return size_for(v, [&](auto cv) {
        return VerifyImpl<decltype(cv)>::ser_grouped_mixed_workspace_bytes(v, m_of, count, group);
    });
}

extern "C" int bpp_range_verify_batch_serialized_grouped_mixed_device(bpp_verifier* v, const void* d_proofs,
                                                                      const void* d_commitments, const uint32_t* m_of,
                                                                      size_t count, int flags, const uint8_t* weight_key,
                                                                      uint64_t index_base, uint32_t group, uint32_t* d_ok,
                                                                      uint64_t* stats, void* d_workspace,
                                                                      size_t workspace_bytes, void* stream) {
    VerifyArgs a;
    a.proofs = static_cast<const uint8_t*>(d_proofs); a.commitments = static_cast<const uint8_t*>(d_commitments);
    a.m_of = m_of; a.count = count; a.weight_key = weight_key; a.index_base = index_base; a.group = group;
    a.ok = d_ok; a.stats = stats;
    if (int rc = verify_args(VERIFY_SER_GROUPED_MIXED, facts(v), flags, a, d_workspace)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int {
        return VerifyImpl<decltype(cv)>::run_serialized_grouped_mixed(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

// ---- proving blocks of mixed aggregation sizes (impl_prove_batch.hpp prove_mixed; the checks: prove_args above) ----------
extern "C" size_t bpp_prover_mixed_workspace_bytes(const bpp_verifier* engine, const uint32_t* m_of, size_t count) {
    if ((count && !m_of) || count > 0x7fffffffu / 64) return 0;
    return size_for(engine, [&](auto cv) { return ProveBatchImpl<decltype(cv)>::prove_mixed_workspace_bytes(engine, m_of, count, false); });
}

extern "C" int bpp_range_prove_batch_mixed_device(bpp_verifier* engine, const uint64_t* d_v, const uint64_t* d_gamma,
                                                  const uint32_t* m_of, size_t count, int flags, const uint8_t* blind_key,
                                                  uint64_t index_base, const uint64_t* d_blinding, uint64_t* d_out_points,
                                                  uint64_t* d_out_scalars, uint64_t* d_out_challenges, void* d_workspace,
                                                  size_t workspace_bytes, void* stream) {
    ProveArgs a;
    a.values = d_v; a.gammas = d_gamma; a.m_of = m_of; a.count = count;
    a.blind_key = blind_key; a.index_base = index_base; a.blinding = d_blinding;
    a.out_points = d_out_points; a.out_scalars = d_out_scalars; a.out_challenges = d_out_challenges;
    if (int rc = prove_args(engine, PROVE_MIXED_DEVICE, flags, a, d_v && d_gamma && m_of && d_out_points && d_out_scalars && d_workspace))
        return rc;
    if (count == 0) return BPP_OK;
    return on_ctx(engine->ctx, {count, "count"}, [&](auto cv) -> int {
        return ProveBatchImpl<decltype(cv)>::prove_device(engine, a, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream));
    });
}

extern "C" size_t bpp_prover_serialized_mixed_workspace_bytes(const bpp_verifier* engine, const uint32_t* m_of, size_t count) {
    if ((count && !m_of) || count > 0x7fffffffu / 64) return 0;
    return size_for(engine, [&](auto cv) { return ProveBatchImpl<decltype(cv)>::prove_mixed_workspace_bytes(engine, m_of, count, true); });
}

extern "C" int bpp_range_prove_batch_serialized_mixed_device(bpp_verifier* engine, const uint64_t* d_v, const uint64_t* d_gamma,
                                                             const uint32_t* m_of, size_t count, int flags,
                                                             const uint8_t* blind_key, uint64_t index_base,
                                                             const uint64_t* d_blinding, void* d_out_proofs,
                                                             void* d_out_commitments, void* d_workspace, size_t workspace_bytes,
                                                             void* stream) {
    ProveArgs a;
    a.values = d_v; a.gammas = d_gamma; a.m_of = m_of; a.count = count;
    a.blind_key = blind_key; a.index_base = index_base; a.blinding = d_blinding;
    a.out_proofs = static_cast<uint8_t*>(d_out_proofs); a.out_commitments = static_cast<uint8_t*>(d_out_commitments);
    if (int rc = prove_args(engine, PROVE_SER_DEVICE, flags, a, d_v && d_gamma && m_of && d_out_proofs && d_out_commitments && d_workspace))
        return rc;
    if (count == 0) return BPP_OK;
    return on_ctx(engine->ctx, {count, "count"}, [&](auto cv) -> int {
        return ProveBatchImpl<decltype(cv)>::prove_device(engine, a, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream));
    });
}

// host buffers in, host buffers out: the device paths above between copies
extern "C" int bpp_range_prove_batch_mixed(bpp_verifier* engine, const uint64_t* v, const uint64_t* gamma, const uint32_t* m_of,
                                           size_t count, int flags, const uint8_t* blind_key, uint64_t index_base,
                                           uint64_t* out_points, uint64_t* out_scalars, uint64_t* out_challenges) {
    ProveArgs a;
    a.values = v; a.gammas = gamma; a.m_of = m_of; a.count = count; a.blind_key = blind_key; a.index_base = index_base;
    a.out_points = out_points; a.out_scalars = out_scalars; a.out_challenges = out_challenges;
    if (int rc = prove_args(engine, PROVE_MIXED_HOST, flags, a, v && gamma && m_of && out_points && out_scalars)) return rc;
    if (count == 0) return BPP_OK;
    return on_ctx(engine->ctx, {count, "count"}, [&](auto cv) -> int { return ProveBatchImpl<decltype(cv)>::prove_host(engine, a); });
}

extern "C" int bpp_range_prove_batch_serialized_mixed(bpp_verifier* engine, const uint64_t* v, const uint64_t* gamma,
                                                      const uint32_t* m_of, size_t count, int flags, const uint8_t* blind_key,
                                                      uint64_t index_base, uint8_t* out_proofs, uint8_t* out_commitments) {
    ProveArgs a;
    a.values = v; a.gammas = gamma; a.m_of = m_of; a.count = count; a.blind_key = blind_key; a.index_base = index_base;
    a.out_proofs = out_proofs; a.out_commitments = out_commitments;
    if (int rc = prove_args(engine, PROVE_SER_HOST, flags, a, v && gamma && m_of && out_proofs && out_commitments)) return rc;
    if (count == 0) return BPP_OK;
    if (int rc = container_version_ok(container_point_size(engine->ctx.curve, (int)a.version))) return rc;
    return on_ctx(engine->ctx, {count, "count"}, [&](auto cv) -> int { return ProveBatchImpl<decltype(cv)>::prove_host(engine, a); });
}

// ---- commitments for a block of amounts through the engine's tables (commit.hpp; RangeProver::commit, range/prover.rs:28-42;
// flags = 0 keeps the `v as i32` of range/prover.rs:37, BPP_PROVE_AMOUNT64 commits the whole u64) ----------------------------
extern "C" int bpp_commit_batch_device(bpp_verifier* engine, const uint64_t* d_v, const uint64_t* d_gamma, size_t count, int flags,
                                       uint64_t* d_out_V, void* stream) {
    if (!engine) return fail(BPP_E_ARG, "null argument");
    if (flags & ~BPP_PROVE_AMOUNT64) return fail(BPP_E_ARG, "unknown flag");
    if (count == 0) return BPP_OK;
    if (!d_v || !d_gamma || !d_out_V) return fail(BPP_E_ARG, "null argument");
    return on_ctx(engine->ctx, {count, "count"}, [&](auto cv) -> int {
        return CommitImpl<decltype(cv)>::commit_batch_device(engine, d_v, d_gamma, count, (flags & BPP_PROVE_AMOUNT64) != 0, d_out_V,
                                                             static_cast<hipStream_t>(stream));
    });
}

extern "C" int bpp_commit_batch(bpp_verifier* engine, const uint64_t* v, const uint64_t* gamma, size_t count, int flags,
                                uint64_t* out_V) {
    if (!engine) return fail(BPP_E_ARG, "null argument");
    if (flags & ~BPP_PROVE_AMOUNT64) return fail(BPP_E_ARG, "unknown flag");
    if (count == 0) return BPP_OK;
    if (!v || !gamma || !out_V) return fail(BPP_E_ARG, "null argument");
    return on_ctx(engine->ctx, {count, "count"}, [&](auto cv) -> int {
        return CommitImpl<decltype(cv)>::commit_batch(engine, v, gamma, count, (flags & BPP_PROVE_AMOUNT64) != 0, out_V);
    });
}

// ---- mask recovery and scanning (recover.hpp; the quantities inverted: range/mod.rs:159-172, wip.rs:94-95,175-227), under
// one key and under many (recover_keys.hpp: the front and the inversions once, n_keys x count pairs).  Each entry fills its
// record and passes scan_args (scan_args.hpp), which answers an empty call itself ----
extern "C" size_t bpp_recover_mixed_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count) {
    if ((count && !m_of) || count > ONE_LAUNCH || !m_of_wellformed(m_of, count)) return 0;
    return size_for(v, [&](auto cv) { return RecoverImpl<decltype(cv)>::recover_workspace_bytes(v, m_of, count); });
}

extern "C" int bpp_range_recover_masks_mixed_device(bpp_verifier* v, const uint64_t* d_scalars, const uint32_t* m_of, size_t count,
                                                    const uint64_t* d_challenges, const uint8_t* blind_key, uint64_t index_base,
                                                    const uint64_t* d_index, const uint64_t* d_blinding, uint64_t* d_out_masks,
                                                    void* d_workspace, size_t workspace_bytes, void* stream) {
    ScanArgs a;
    a.scalars = d_scalars; a.m_of = m_of; a.count = count; a.challenges = d_challenges;
    a.blind_key = blind_key; a.index_base = index_base; a.index = d_index; a.blinding = d_blinding; a.out_masks = d_out_masks;
    if (int rc = scan_args(SCAN_RECOVER_DEVICE, v != nullptr, 0, a, d_workspace, workspace_bytes)) return answered(rc);
    return on_ctx(v->ctx, {count, "count"}, [&](auto cv) -> int {
        return RecoverImpl<decltype(cv)>::recover_masks_mixed(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

// host buffers in, host masks out: the device path above between copies
extern "C" int bpp_range_recover_masks_mixed(bpp_verifier* v, const uint64_t* scalars, const uint32_t* m_of, size_t count,
                                             const uint64_t* challenges, const uint8_t* blind_key, uint64_t index_base,
                                             const uint64_t* index, const uint64_t* blinding, uint64_t* out_masks) {
    ScanArgs a;
    a.scalars = scalars; a.m_of = m_of; a.count = count; a.challenges = challenges;
    a.blind_key = blind_key; a.index_base = index_base; a.index = index; a.blinding = blinding; a.out_masks = out_masks;
    if (int rc = scan_args(SCAN_RECOVER_HOST, v != nullptr, 0, a, nullptr, 0)) return answered(rc);
    return on_ctx(v->ctx, {count, "count"}, [&](auto cv) -> int { return RecoverImpl<decltype(cv)>::recover_masks_mixed_host(v, a); });
}

extern "C" size_t bpp_scan_serialized_mixed_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count) {
    if ((count && !m_of) || count > ONE_LAUNCH || !m_of_wellformed(m_of, count)) return 0;
    return size_for(v, [&](auto cv) { return RecoverImpl<decltype(cv)>::scan_workspace_bytes(v, m_of, count); });
}

extern "C" int bpp_range_scan_serialized_mixed_device(bpp_verifier* v, const void* d_proofs, const void* d_commitments,
                                                      const uint32_t* m_of, size_t count, int flags, const uint8_t* blind_key,
                                                      uint64_t index_base, const uint64_t* d_index, const uint64_t* d_blinding,
                                                      const uint64_t* d_amounts, uint64_t* d_out_masks, uint32_t* d_status,
                                                      void* d_workspace, size_t workspace_bytes, void* stream) {
    ScanArgs a;
    a.proofs = static_cast<const uint8_t*>(d_proofs); a.commitments = static_cast<const uint8_t*>(d_commitments);
    a.m_of = m_of; a.count = count; a.blind_key = blind_key; a.index_base = index_base; a.index = d_index; a.blinding = d_blinding;
    a.amounts = d_amounts; a.out_masks = d_out_masks; a.out_status = d_status;
    if (int rc = scan_args(SCAN_ONE_KEY_DEVICE, v != nullptr, flags, a, d_workspace, workspace_bytes)) return answered(rc);
    return on_ctx(v->ctx, {count, "count"}, [&](auto cv) -> int {
        return RecoverImpl<decltype(cv)>::scan_serialized_mixed(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

// host buffers in, host masks and statuses out: the device path above between copies
extern "C" int bpp_range_scan_serialized_mixed(bpp_verifier* v, const uint8_t* proofs, const uint8_t* commitments,
                                               const uint32_t* m_of, size_t count, int flags, const uint8_t* blind_key,
                                               uint64_t index_base, const uint64_t* index, const uint64_t* blinding,
                                               const uint64_t* amounts, uint64_t* out_masks, uint32_t* out_status) {
    ScanArgs a;
    a.proofs = proofs; a.commitments = commitments; a.m_of = m_of; a.count = count;
    a.blind_key = blind_key; a.index_base = index_base; a.index = index; a.blinding = blinding;
    a.amounts = amounts; a.out_masks = out_masks; a.out_status = out_status;
    if (int rc = scan_args(SCAN_ONE_KEY_HOST, v != nullptr, flags, a, nullptr, 0)) return answered(rc);
    return on_ctx(v->ctx, {count, "count"}, [&](auto cv) -> int { return RecoverImpl<decltype(cv)>::scan_serialized_mixed_host(v, a); });
}

extern "C" size_t bpp_scan_serialized_mixed_keys_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count,
                                                                 size_t n_keys) {
    if ((count && !m_of) || !pairs_bounded(n_keys, count) || !m_of_wellformed(m_of, count)) return 0;
    return size_for(v, [&](auto cv) { return RecoverKeysImpl<decltype(cv)>::workspace_bytes(v, m_of, count); });
}

extern "C" int bpp_range_scan_serialized_mixed_keys_device(bpp_verifier* v, const void* d_proofs, const void* d_commitments,
                                                           const uint32_t* m_of, size_t count, int flags, const uint8_t* d_keys,
                                                           size_t n_keys, uint64_t index_base, const uint64_t* d_index,
                                                           const uint64_t* d_amounts, uint64_t* d_out_masks, uint32_t* d_status,
                                                           void* d_workspace, size_t workspace_bytes, void* stream) {
    ScanArgs a;
    a.proofs = static_cast<const uint8_t*>(d_proofs); a.commitments = static_cast<const uint8_t*>(d_commitments);
    a.m_of = m_of; a.count = count; a.keys = d_keys; a.n_keys = n_keys; a.index_base = index_base; a.index = d_index;
    a.amounts = d_amounts; a.out_masks = d_out_masks; a.out_status = d_status;
    if (int rc = scan_args(SCAN_MANY_KEYS_DEVICE, v != nullptr, flags, a, d_workspace, workspace_bytes)) return answered(rc);
    return on_ctx(v->ctx, {count, "count"}, [&](auto cv) -> int {
        return RecoverKeysImpl<decltype(cv)>::scan(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

// host buffers in (keys, index and amounts included), host masks and statuses out: the device path above between copies
extern "C" int bpp_range_scan_serialized_mixed_keys(bpp_verifier* v, const uint8_t* proofs, const uint8_t* commitments,
                                                    const uint32_t* m_of, size_t count, int flags, const uint8_t* keys,
                                                    size_t n_keys, uint64_t index_base, const uint64_t* index,
                                                    const uint64_t* amounts, uint64_t* out_masks, uint32_t* out_status) {
    ScanArgs a;
    a.proofs = proofs; a.commitments = commitments; a.m_of = m_of; a.count = count;
    a.keys = keys; a.n_keys = n_keys; a.index_base = index_base; a.index = index;
    a.amounts = amounts; a.out_masks = out_masks; a.out_status = out_status;
    if (int rc = scan_args(SCAN_MANY_KEYS_HOST, v != nullptr, flags, a, nullptr, 0)) return answered(rc);
    return on_ctx(v->ctx, {count, "count"}, [&](auto cv) -> int { return RecoverKeysImpl<decltype(cv)>::scan_host(v, a); });
}

// ---- sealed amounts, view tags, and verifying a block while listing the outputs of many keys, with tags or without
// (find.hpp) ----
namespace {
// The checks of the four entries that expand one key over `count` outputs (seal and tag, device and host); count = 0 passes
// them and is answered by the entry.  buffers: whether every buffer that a count above zero reads or writes, the optional
// index aside, is there.
int key_stream_args(const bpp_ctx* ctx, const uint8_t* blind_key, size_t count, bool buffers) noexcept {
    if (!ctx || !blind_key) return fail(BPP_E_ARG, "null argument");
    if (count == 0) return BPP_OK;
    if (!buffers) return fail(BPP_E_ARG, "null argument");
    if (count > 0x7fffffffu / 64) return fail(BPP_E_ARG, "count too large for one launch");
    return BPP_OK;
}

// What a find entry returns when find_args (scan_args.hpp) did not say go on: its error, or for an empty call BPP_OK behind
// the counts it answers with -- no proof: no verdict, no candidate, no hit -- zeroed on the device or on the host
int find_nothing(int rc, const bpp_verifier* v, const FindArgs& a, bool device, void* stream) noexcept {
    if (rc != SCAN_ANSWERED) return rc;
    if (!device) {
        *a.n_hits = 0;
        if (a.n_candidates) *a.n_candidates = 0;
        return BPP_OK;
    }
    return on_device(v->ctx.device, [&]() -> int {
        HIPCHK(zero_words_async(a.n_hits, 4, hip(stream)));
        if (a.n_candidates) HIPCHK(zero_words_async(a.n_candidates, 4, hip(stream)));
        return BPP_OK;
    });
}
}  // namespace

extern "C" int bpp_amounts_seal_device(bpp_ctx* ctx, const uint8_t* blind_key, uint64_t index_base, const uint64_t* d_index,
                                       const uint64_t* d_in, size_t count, uint64_t* d_out, void* stream) {
    if (int rc = key_stream_args(ctx, blind_key, count, d_in && d_out)) return rc;
    if (count == 0) return BPP_OK;
    return on_ctx(*ctx, {count, "count"}, [&](auto cv) -> int {
        return FindImpl<decltype(cv)>::seal(blind_key, index_base, d_index, d_in, count, d_out, static_cast<hipStream_t>(stream));
    });
}

extern "C" int bpp_amounts_seal(bpp_ctx* ctx, const uint8_t* blind_key, uint64_t index_base, const uint64_t* index,
                                const uint64_t* in, size_t count, uint64_t* out) {
    if (int rc = key_stream_args(ctx, blind_key, count, in && out)) return rc;
    if (count == 0) return BPP_OK;
    return on_ctx(*ctx, {count, "count"}, [&](auto cv) -> int {
        return FindImpl<decltype(cv)>::seal_host(blind_key, index_base, index, in, count, out);
    });
}

extern "C" int bpp_view_tags_device(bpp_ctx* ctx, const uint8_t* blind_key, uint64_t index_base, const uint64_t* d_index,
                                    size_t count, uint8_t* d_out, void* stream) {
    if (int rc = key_stream_args(ctx, blind_key, count, d_out != nullptr)) return rc;
    if (count == 0) return BPP_OK;
    return on_ctx(*ctx, {count, "count"}, [&](auto cv) -> int {
        return FindImpl<decltype(cv)>::tags(blind_key, index_base, d_index, count, d_out, static_cast<hipStream_t>(stream));
    });
}

extern "C" int bpp_view_tags(bpp_ctx* ctx, const uint8_t* blind_key, uint64_t index_base, const uint64_t* index, size_t count,
                             uint8_t* out) {
    if (int rc = key_stream_args(ctx, blind_key, count, out != nullptr)) return rc;
    if (count == 0) return BPP_OK;
    return on_ctx(*ctx, {count, "count"}, [&](auto cv) -> int {
        return FindImpl<decltype(cv)>::tags_host(blind_key, index_base, index, count, out);
    });
}

extern "C" size_t bpp_verify_find_serialized_mixed_keys_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count,
                                                                        size_t n_keys) {
    if ((count && !m_of) || !pairs_bounded(n_keys, count) || !m_of_wellformed(m_of, count)) return 0;
    return size_for(v, [&](auto cv) { return FindImpl<decltype(cv)>::workspace_bytes(v, m_of, count, n_keys, FIND_REWIND); });
}

extern "C" size_t bpp_verify_find_tagged_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, size_t n_keys) {
    if ((count && !m_of) || !pairs_bounded(n_keys, count) || !m_of_wellformed(m_of, count)) return 0;
    return size_for(v, [&](auto cv) { return FindImpl<decltype(cv)>::workspace_bytes(v, m_of, count, n_keys, FIND_REWIND_TAGGED); });
}

extern "C" int bpp_range_verify_find_serialized_mixed_keys_device(bpp_verifier* v, const void* d_proofs, const void* d_commitments,
                                                                  const uint32_t* m_of, size_t count, int flags,
                                                                  const uint8_t* d_keys, size_t n_keys, uint64_t index_base,
                                                                  const uint64_t* d_index, const uint64_t* d_amounts,
                                                                  uint32_t* d_ok, uint32_t* d_hits, size_t max_hits,
                                                                  uint32_t* d_n_hits, void* d_workspace, size_t workspace_bytes,
                                                                  void* stream) {
    FindArgs a{static_cast<const uint8_t*>(d_proofs), static_cast<const uint8_t*>(d_commitments), m_of, count, d_keys, n_keys,
               index_base, d_index, d_amounts, d_ok, d_hits, max_hits, d_n_hits, FIND_REWIND, nullptr, nullptr};
    if (int rc = find_args(v != nullptr, flags, a, true, d_workspace, workspace_bytes)) return find_nothing(rc, v, a, true, stream);
    return on_ctx(v->ctx, {count, "count"}, [&](auto cv) -> int {
        return FindImpl<decltype(cv)>::find(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

// host buffers in (keys, index and amounts included), host verdicts and hit records out: the device path above between copies
extern "C" int bpp_range_verify_find_serialized_mixed_keys(bpp_verifier* v, const uint8_t* proofs, const uint8_t* commitments,
                                                           const uint32_t* m_of, size_t count, int flags, const uint8_t* keys,
                                                           size_t n_keys, uint64_t index_base, const uint64_t* index,
                                                           const uint64_t* amounts, uint32_t* out_ok, uint32_t* out_hits,
                                                           size_t max_hits, uint32_t* out_n_hits) {
    FindArgs a{proofs, commitments, m_of,     count,    keys,       n_keys, index_base, index,
               amounts, out_ok,     out_hits, max_hits, out_n_hits, FIND_REWIND, nullptr, nullptr};
    if (int rc = find_args(v != nullptr, flags, a, false, nullptr, 0)) return find_nothing(rc, v, a, false, nullptr);
    return on_ctx(v->ctx, {count, "count"}, [&](auto cv) -> int { return FindImpl<decltype(cv)>::find_host(v, a); });
}

extern "C" int bpp_range_verify_find_tagged_serialized_mixed_keys_device(
    bpp_verifier* v, const void* d_proofs, const void* d_commitments, const uint32_t* m_of, size_t count, int flags,
    const uint8_t* d_keys, size_t n_keys, uint64_t index_base, const uint64_t* d_index, const uint64_t* d_amounts, uint32_t* d_ok,
    uint32_t* d_hits, size_t max_hits, uint32_t* d_n_hits, const uint8_t* d_tags, uint32_t* d_n_candidates, void* d_workspace,
    size_t workspace_bytes, void* stream) {
    FindArgs a{static_cast<const uint8_t*>(d_proofs), static_cast<const uint8_t*>(d_commitments), m_of, count, d_keys, n_keys,
               index_base, d_index, d_amounts, d_ok, d_hits, max_hits, d_n_hits, FIND_REWIND_TAGGED, d_tags, d_n_candidates};
    if (int rc = find_args(v != nullptr, flags, a, true, d_workspace, workspace_bytes)) return find_nothing(rc, v, a, true, stream);
    return on_ctx(v->ctx, {count, "count"}, [&](auto cv) -> int {
        return FindImpl<decltype(cv)>::find(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

// host buffers in (keys, index, amounts and tags included), host verdicts, hit records and counts out
extern "C" int bpp_range_verify_find_tagged_serialized_mixed_keys(
    bpp_verifier* v, const uint8_t* proofs, const uint8_t* commitments, const uint32_t* m_of, size_t count, int flags,
    const uint8_t* keys, size_t n_keys, uint64_t index_base, const uint64_t* index, const uint64_t* amounts, uint32_t* out_ok,
    uint32_t* out_hits, size_t max_hits, uint32_t* out_n_hits, const uint8_t* tags, uint32_t* out_n_candidates) {
    FindArgs a{proofs, commitments, m_of,     count,    keys,       n_keys, index_base, index,
               amounts, out_ok,     out_hits, max_hits, out_n_hits, FIND_REWIND_TAGGED, tags, out_n_candidates};
    if (int rc = find_args(v != nullptr, flags, a, false, nullptr, 0)) return find_nothing(rc, v, a, false, nullptr);
    return on_ctx(v->ctx, {count, "count"}, [&](auto cv) -> int { return FindImpl<decltype(cv)>::find_host(v, a); });
}

// ---- outputs with masks derived from their recipients' keys: making them, and verifying a block while listing each
// key's outputs, aggregated proofs included (outputs.hpp) ----
namespace {
// the checks of the sender's two entries; n_out = 0 passes them and is answered by the entry
int outputs_make_args(const bpp_ctx* ctx, const void* keys, const void* index, const void* j, const void* amounts, size_t n_out,
                      const void* out_masks, const void* out_sealed, const void* out_tags, bool device) noexcept {
    if (!ctx) return fail(BPP_E_ARG, "null argument");
    if (!out_masks && !out_sealed && !out_tags) return fail(BPP_E_ARG, "null argument: nothing to make");
    if (n_out == 0) return BPP_OK;
    if (!keys || !index || !j || !amounts) return fail(BPP_E_ARG, "null argument");
    if (device && (reinterpret_cast<uintptr_t>(keys) & 3)) return fail(BPP_E_ARG, "d_keys must be 4-byte aligned");
    if (n_out > 0x7fffffffu / 64) return fail(BPP_E_ARG, "n_out too large for one launch");
    return BPP_OK;
}
}  // namespace

extern "C" int bpp_outputs_make_device(bpp_ctx* ctx, const uint8_t* d_keys, const uint64_t* d_index, const uint32_t* d_j,
                                       const uint64_t* d_amounts, size_t n_out, uint64_t* d_out_masks, uint64_t* d_out_sealed,
                                       uint8_t* d_out_tags, void* stream) {
    if (int rc = outputs_make_args(ctx, d_keys, d_index, d_j, d_amounts, n_out, d_out_masks, d_out_sealed, d_out_tags, true)) return rc;
    if (n_out == 0) return BPP_OK;
    return on_ctx(*ctx, {n_out, "n_out"}, [&](auto cv) -> int {
        return OutputsImpl<decltype(cv)>::make(d_keys, d_index, d_j, d_amounts, n_out, d_out_masks, d_out_sealed, d_out_tags,
                                               static_cast<hipStream_t>(stream));
    });
}

// host buffers in, host masks, sealed amounts and tags out: the device path above between copies
extern "C" int bpp_outputs_make(bpp_ctx* ctx, const uint8_t* keys, const uint64_t* index, const uint32_t* j, const uint64_t* amounts,
                                size_t n_out, uint64_t* out_masks, uint64_t* out_sealed, uint8_t* out_tags) {
    if (int rc = outputs_make_args(ctx, keys, index, j, amounts, n_out, out_masks, out_sealed, out_tags, false)) return rc;
    if (n_out == 0) return BPP_OK;
    return on_ctx(*ctx, {n_out, "n_out"}, [&](auto cv) -> int {
        return OutputsImpl<decltype(cv)>::make_host(keys, index, j, amounts, n_out, out_masks, out_sealed, out_tags);
    });
}

extern "C" size_t bpp_verify_find_outputs_workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, size_t n_keys) {
    if ((count && !m_of) || !pairs_bounded(n_keys, pair_units(m_of, count, true)) || !m_of_wellformed(m_of, count)) return 0;
    return size_for(v, [&](auto cv) { return OutputsImpl<decltype(cv)>::workspace_bytes(v, m_of, count, n_keys); });
}

extern "C" int bpp_range_verify_find_outputs_serialized_mixed_keys_device(
    bpp_verifier* v, const void* d_proofs, const void* d_commitments, const uint32_t* m_of, size_t count, int flags,
    const uint8_t* d_keys, size_t n_keys, uint64_t index_base, const uint64_t* d_index, const uint64_t* d_sealed,
    const uint8_t* d_tags, uint32_t* d_ok, uint32_t* d_hits, size_t max_hits, uint32_t* d_n_hits, uint32_t* d_n_candidates,
    void* d_workspace, size_t workspace_bytes, void* stream) {
    FindArgs a{static_cast<const uint8_t*>(d_proofs), static_cast<const uint8_t*>(d_commitments), m_of, count, d_keys, n_keys,
               index_base, d_index, d_sealed, d_ok, d_hits, max_hits, d_n_hits, FIND_PER_OUTPUT, d_tags, d_n_candidates};
    if (int rc = find_args(v != nullptr, flags, a, true, d_workspace, workspace_bytes)) return find_nothing(rc, v, a, true, stream);
    return on_ctx(v->ctx, {count, "count"}, [&](auto cv) -> int {
        return OutputsImpl<decltype(cv)>::find(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

// host buffers in (keys, index, sealed amounts and tags included), host verdicts, hit records and counts out
extern "C" int bpp_range_verify_find_outputs_serialized_mixed_keys(
    bpp_verifier* v, const uint8_t* proofs, const uint8_t* commitments, const uint32_t* m_of, size_t count, int flags,
    const uint8_t* keys, size_t n_keys, uint64_t index_base, const uint64_t* index, const uint64_t* sealed, const uint8_t* tags,
    uint32_t* out_ok, uint32_t* out_hits, size_t max_hits, uint32_t* out_n_hits, uint32_t* out_n_candidates) {
    FindArgs a{proofs, commitments, m_of,     count,    keys,       n_keys,          index_base, index,
               sealed, out_ok,      out_hits, max_hits, out_n_hits, FIND_PER_OUTPUT, tags,       out_n_candidates};
    if (int rc = find_args(v != nullptr, flags, a, false, nullptr, 0)) return find_nothing(rc, v, a, false, nullptr);
    return on_ctx(v->ctx, {count, "count"}, [&](auto cv) -> int { return OutputsImpl<decltype(cv)>::find_host(v, a); });
}

// ---- proofs over any number of outputs (outs_plan.hpp): proof i covers outs_of[i] outputs, is the proof of shape
// (n, 2^ceil(log2 outs_of[i])) over values and masks padded with zeros, and the streams carry the real outputs alone.  The
// entries of the serialized mixed calls with outs_of in m_of's place: the same records, the same checks, the same fronts ----
extern "C" int bpp_outs_shapes(const uint32_t* outs_of, size_t count, size_t cap_m, uint32_t* m_of_out) {
    if (count && (!outs_of || !m_of_out)) return fail(BPP_E_ARG, "null argument");
    return guarded({count, "count"}, [&] { return outs_shapes(outs_of, count, cap_m, m_of_out); });
}

extern "C" size_t bpp_prover_serialized_outs_workspace_bytes(const bpp_verifier* engine, const uint32_t* outs_of, size_t count) {
    if (!outs_wellformed(outs_of, count)) return 0;
    return size_for(engine, [&](auto cv) {
        return ProveBatchImpl<decltype(cv)>::prove_mixed_workspace_bytes(engine, nullptr, count, true, outs_of);
    });
}

extern "C" int bpp_range_prove_batch_serialized_outs_device(bpp_verifier* engine, const uint64_t* d_v, const uint64_t* d_gamma,
                                                            const uint32_t* outs_of, size_t count, int flags,
                                                            const uint8_t* blind_key, uint64_t index_base,
                                                            const uint64_t* d_blinding, void* d_out_proofs,
                                                            void* d_out_commitments, void* d_workspace, size_t workspace_bytes,
                                                            void* stream) {
    ProveArgs a;
    a.values = d_v; a.gammas = d_gamma; a.outs_of = outs_of; a.count = count;
    a.blind_key = blind_key; a.index_base = index_base; a.blinding = d_blinding;
    a.out_proofs = static_cast<uint8_t*>(d_out_proofs); a.out_commitments = static_cast<uint8_t*>(d_out_commitments);
    if (int rc = prove_args(engine, PROVE_SER_DEVICE, flags, a, d_v && d_gamma && outs_of && d_out_proofs && d_out_commitments && d_workspace))
        return rc;
    if (count == 0) return BPP_OK;
    return on_ctx(engine->ctx, {count, "count"}, [&](auto cv) -> int {
        return ProveBatchImpl<decltype(cv)>::prove_device(engine, a, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream));
    });
}

// host buffers in, host buffers out: the device path above between copies
extern "C" int bpp_range_prove_batch_serialized_outs(bpp_verifier* engine, const uint64_t* v, const uint64_t* gamma,
                                                     const uint32_t* outs_of, size_t count, int flags, const uint8_t* blind_key,
                                                     uint64_t index_base, uint8_t* out_proofs, uint8_t* out_commitments) {
    ProveArgs a;
    a.values = v; a.gammas = gamma; a.outs_of = outs_of; a.count = count; a.blind_key = blind_key; a.index_base = index_base;
    a.out_proofs = out_proofs; a.out_commitments = out_commitments;
    if (int rc = prove_args(engine, PROVE_SER_HOST, flags, a, v && gamma && outs_of && out_proofs && out_commitments)) return rc;
    if (count == 0) return BPP_OK;
    if (int rc = container_version_ok(container_point_size(engine->ctx.curve, (int)a.version))) return rc;
    return on_ctx(engine->ctx, {count, "count"}, [&](auto cv) -> int { return ProveBatchImpl<decltype(cv)>::prove_host(engine, a); });
}

extern "C" size_t bpp_verifier_serialized_outs_workspace_bytes(const bpp_verifier* v, const uint32_t* outs_of, size_t count) {
    if (!outs_wellformed(outs_of, count)) return 0;
    return size_for(v, [&](auto cv) { return VerifyImpl<decltype(cv)>::ser_mixed_workspace_bytes(v, nullptr, count, outs_of); });
}

extern "C" int bpp_range_verify_batch_serialized_outs_device(bpp_verifier* v, const void* d_proofs, const void* d_commitments,
                                                             const uint32_t* outs_of, size_t count, int flags, uint32_t* d_ok,
                                                             void* d_workspace, size_t workspace_bytes, void* stream) {
    VerifyArgs a;
    a.proofs = static_cast<const uint8_t*>(d_proofs); a.commitments = static_cast<const uint8_t*>(d_commitments);
    a.outs_of = outs_of; a.count = count; a.ok = d_ok;
    if (int rc = verify_args(VERIFY_SER_MIXED, facts(v), flags, a, d_workspace)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int {
        return VerifyImpl<decltype(cv)>::run_serialized_mixed(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

// host buffers in, host verdicts out: the device path above between two copies
extern "C" int bpp_range_verify_batch_serialized_outs(bpp_verifier* v, const uint8_t* proofs, const uint8_t* commitments,
                                                      const uint32_t* outs_of, size_t count, int flags, uint32_t* out_ok) {
    VerifyArgs a;
    a.proofs = proofs; a.commitments = commitments; a.outs_of = outs_of; a.count = count; a.ok = out_ok;
    if (int rc = verify_args(VERIFY_HOST_SER_MIXED, facts(v), flags, a, nullptr)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int { return VerifyImpl<decltype(cv)>::verify_host(v, a, HOST_SERIALIZED_MIXED, flags); });
}

extern "C" size_t bpp_verifier_serialized_grouped_outs_workspace_bytes(const bpp_verifier* v, const uint32_t* outs_of, size_t count,
                                                                       uint32_t group) {
    if (!outs_wellformed(outs_of, count)) return 0;
    return size_for(v, [&](auto cv) {
        return VerifyImpl<decltype(cv)>::ser_grouped_mixed_workspace_bytes(v, nullptr, count, group, outs_of);
    });
}

extern "C" int bpp_range_verify_batch_serialized_grouped_outs_device(bpp_verifier* v, const void* d_proofs,
                                                                     const void* d_commitments, const uint32_t* outs_of,
                                                                     size_t count, int flags, const uint8_t* weight_key,
                                                                     uint64_t index_base, uint32_t group, uint32_t* d_ok,
                                                                     uint64_t* stats, void* d_workspace, size_t workspace_bytes,
                                                                     void* stream) {
    VerifyArgs a;
    a.proofs = static_cast<const uint8_t*>(d_proofs); a.commitments = static_cast<const uint8_t*>(d_commitments);
    a.outs_of = outs_of; a.count = count; a.weight_key = weight_key; a.index_base = index_base; a.group = group;
    a.ok = d_ok; a.stats = stats;
    if (int rc = verify_args(VERIFY_SER_GROUPED_MIXED, facts(v), flags, a, d_workspace)) return answered(rc);
    return on_ctx(v->ctx, [&](auto cv) -> int {
        return VerifyImpl<decltype(cv)>::run_serialized_grouped_mixed(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

extern "C" size_t bpp_verify_find_outputs_outs_workspace_bytes(const bpp_verifier* v, const uint32_t* outs_of, size_t count,
                                                               size_t n_keys) {
    if (!outs_wellformed(outs_of, count) || !pairs_bounded(n_keys, pair_units(outs_of, count, true))) return 0;
    return size_for(v, [&](auto cv) { return OutputsImpl<decltype(cv)>::workspace_bytes(v, nullptr, count, n_keys, outs_of); });
}

extern "C" int bpp_range_verify_find_outputs_serialized_outs_keys_device(
    bpp_verifier* v, const void* d_proofs, const void* d_commitments, const uint32_t* outs_of, size_t count, int flags,
    const uint8_t* d_keys, size_t n_keys, uint64_t index_base, const uint64_t* d_index, const uint64_t* d_sealed,
    const uint8_t* d_tags, uint32_t* d_ok, uint32_t* d_hits, size_t max_hits, uint32_t* d_n_hits, uint32_t* d_n_candidates,
    void* d_workspace, size_t workspace_bytes, void* stream) {
    FindArgs a{static_cast<const uint8_t*>(d_proofs), static_cast<const uint8_t*>(d_commitments), nullptr, count, d_keys, n_keys,
               index_base, d_index, d_sealed, d_ok, d_hits, max_hits, d_n_hits, FIND_PER_OUTPUT, d_tags, d_n_candidates};
    a.outs_of = outs_of;
    if (int rc = find_args(v != nullptr, flags, a, true, d_workspace, workspace_bytes)) return find_nothing(rc, v, a, true, stream);
    return on_ctx(v->ctx, {count, "count"}, [&](auto cv) -> int {
        return OutputsImpl<decltype(cv)>::find(v, a, d_workspace, workspace_bytes, hip(stream));
    });
}

// host buffers in (keys, index, sealed amounts and tags included), host verdicts, hit records and counts out
extern "C" int bpp_range_verify_find_outputs_serialized_outs_keys(
    bpp_verifier* v, const uint8_t* proofs, const uint8_t* commitments, const uint32_t* outs_of, size_t count, int flags,
    const uint8_t* keys, size_t n_keys, uint64_t index_base, const uint64_t* index, const uint64_t* sealed, const uint8_t* tags,
    uint32_t* out_ok, uint32_t* out_hits, size_t max_hits, uint32_t* out_n_hits, uint32_t* out_n_candidates) {
    FindArgs a{proofs, commitments, nullptr,  count,    keys,       n_keys,          index_base, index,
               sealed, out_ok,      out_hits, max_hits, out_n_hits, FIND_PER_OUTPUT, tags,       out_n_candidates};
    a.outs_of = outs_of;
    if (int rc = find_args(v != nullptr, flags, a, false, nullptr, 0)) return find_nothing(rc, v, a, false, nullptr);
    return on_ctx(v->ctx, {count, "count"}, [&](auto cv) -> int { return OutputsImpl<decltype(cv)>::find_host(v, a); });
}

// ---- the verifier pool: one batch sharded over the devices of a node (shard.hpp, pool.hpp; see include/bpp_amd.h) ----
#include "pool.hpp"

extern "C" int bpp_shard_cuts(const uint32_t* m_of, size_t count, size_t world, size_t* out_cuts) {
    return guarded([&] { return shard_cuts(m_of, count, world, out_cuts); });
}

extern "C" int bpp_pool_create(int curve_id, const int* devices, size_t n_dev, const uint64_t* gh, const uint64_t* G,
                               const uint64_t* H, size_t n, size_t m, int window_bits, void** out) {
    if (!out) return fail(BPP_E_ARG, "null out");
    *out = nullptr;
    if (!devices || !gh || !G || !H) return fail(BPP_E_ARG, "null argument");
    if (n_dev == 0 || n_dev > POOL_MAX_SHARDS) return fail(BPP_E_ARG, "n_dev must be in [1, 16]");
    return guarded([&] {
        bpp_pool* pool = nullptr;
        const int rc = pool_create(curve_id, devices, n_dev, gh, G, H, n, m, window_bits, &pool);
        *out = pool;
        return rc;
    });
}
extern "C" void bpp_pool_destroy(void* pool) {
    (void)guarded([&] {
        pool_release(static_cast<bpp_pool*>(pool));
        return BPP_OK;
    });
}
extern "C" size_t bpp_pool_size(const void* pool) {
    size_t r = 0;
    if (pool)
        (void)guarded([&] {
            r = static_cast<const bpp_pool*>(pool)->shards.size();
            return BPP_OK;
        });
    return r;
}
extern "C" int bpp_pool_device(const void* pool, size_t shard) {
    int d = -1;
    if (pool)
        (void)guarded([&] {
            const bpp_pool* p = static_cast<const bpp_pool*>(pool);
            if (shard < p->shards.size()) d = p->shards[shard].device;
            return BPP_OK;
        });
    return d;
}
extern "C" int bpp_pool_verifier(void* pool, size_t shard, bpp_verifier** out) {
    if (!out) return fail(BPP_E_ARG, "null out");
    *out = nullptr;
    if (!pool) return fail(BPP_E_ARG, "null pool");
    return guarded([&] {
        bpp_pool* p = static_cast<bpp_pool*>(pool);
        if (shard >= p->shards.size()) return fail(BPP_E_ARG, "no such shard");
        *out = p->shards[shard].v;
        return BPP_OK;
    });
}

extern "C" int bpp_pool_verify_mixed(void* pool, const uint64_t* points, const uint64_t* scalars, const uint32_t* m_of,
                                     size_t count, uint32_t* out_ok) {
    if (!pool) return fail(BPP_E_ARG, "null pool");
    if (count == 0) return BPP_OK;
    if (!points || !scalars || !out_ok) return fail(BPP_E_ARG, "null argument");
    return guarded({count, "count"}, [&] {
        return pool_verify_mixed(static_cast<bpp_pool*>(pool), points, scalars, m_of, count, out_ok);
    });
}

extern "C" int bpp_pool_verify_serialized_mixed(void* pool, const uint8_t* proofs, const uint8_t* commitments,
                                                const uint32_t* m_of, size_t count, int flags, int mode,
                                                const uint8_t* weight_key, uint64_t index_base, uint32_t group,
                                                uint32_t* out_ok, uint64_t* stats) {
    if (!pool) return fail(BPP_E_ARG, "null pool");
    if (flags & ~(BPP_SER_TRANSCRIPT | BPP_SER_UNCOMPRESSED)) return fail(BPP_E_ARG, "unknown flag");
    if (mode != BPP_POOL_EXACT && mode != BPP_POOL_GROUPED) return fail(BPP_E_ARG, "unknown mode");
    if (mode == BPP_POOL_GROUPED) {
        if (!weight_key) return fail(BPP_E_ARG, "null weight_key: the grouped check needs a weight key");
        if (group < 2 || (group & (group - 1))) return fail(BPP_E_ARG, "group must be a power of two >= 2");
    }
    if (count == 0) {
        if (mode == BPP_POOL_GROUPED && stats) stats[0] = stats[1] = 0;
        return BPP_OK;
    }
    if (!proofs || !commitments || !m_of || !out_ok) return fail(BPP_E_ARG, "null argument");
    return guarded({count, "count"}, [&] {
        return pool_verify_serialized_mixed(static_cast<bpp_pool*>(pool), proofs, commitments, m_of, count, flags, mode,
                                            weight_key, index_base, group, out_ok, stats);
    });
}

extern "C" int bpp_pool_verify_combined(void* pool, const uint64_t* points, const uint64_t* scalars, size_t count,
                                        const uint8_t* weight_key, uint64_t index_base, uint32_t* out_ok) {
    if (!pool || !out_ok) return fail(BPP_E_ARG, "null argument");
    if (!weight_key) return fail(BPP_E_ARG, "null weight_key: the combined check needs a weight key");
    if (count == 0) {
        *out_ok = 0;
        return BPP_OK;
    }
    if (!points || !scalars) return fail(BPP_E_ARG, "null argument");
    return guarded({count, "count"}, [&] {
        return pool_verify_combined(static_cast<bpp_pool*>(pool), points, scalars, count, weight_key, index_base, out_ok);
    });
}
