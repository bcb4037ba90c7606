/*
 * bpp_amd.h -- C ABI of the MI355X-native Bulletproofs+ engine (libbpp_amd.so).
 *
 * This is the drop-in boundary for the reference crate's hot path (gogoex/BulletProofsPlus): every
 * entry point below names the reference interface it replaces (paths relative to /root/reference).
 * The reference has no FFI of its own; its only ABI crossing is Rust -> libmcl inside mcl_rust.
 * Here the crossing moves up to the MulVec / RangeProof level: host -> extern "C" -> HIP.
 * INTEGRATION.md shows the Rust `extern "C"` block and the replacement bodies of
 * `MulVec::calculate`, `RangeProof::{prove,verify}`, `PublicKey::new`, `RangeProver::commit`.
 *
 * Conventions
 *   - plain pointers and sizes only; caller owns every buffer; nothing borrowed outlives a call.
 *   - return value: 0 = Ok(()), 1 = Err(ProofError::VerificationError)
 *     (reference src/errors.rs:14-50; the only variant the path constructs, range/mod.rs:508,
 *     weighted_inner_product_proof.rs:326,336), negative = usage / runtime error (BPP_E_*), where the
 *     reference would panic (mulvec.rs:23-25, range/mod.rs:90-91,252-253, wip.rs:60-67).
 *     Nothing unwinds, nothing is printed.  A failed host allocation returns BPP_E_NOMEM; a count of 2^32 or
 *     more (proofs, points, scalars, generators) returns BPP_E_ARG.
 *   - scalar: 4 x uint64_t little-endian limbs, canonical (non-Montgomery) value; values >= r are
 *     reduced mod r on entry.
 *   - point : (2*L + 1) x uint64_t = affine x (L limbs LE) | y (L limbs LE) | infinity flag (0/1),
 *     canonical coordinates; L = 6 for BLS12-381 G1, 4 for secp256k1 (bpp_point_words()).
 *   - there is no CPU fallback: every call runs HIP kernels on the context's device and fails with
 *     BPP_E_HIP if the device is unusable.
 *   - a context is bound to one device and one thread at a time; contexts are independent.
 */
#ifndef BPP_AMD_H
#define BPP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* curve ids.  BLS12-381 G1 is what the reference's range proof is wired to (src/range/mod.rs:10-15);
 * secp256k1 is its second, in-tree backend (src/secp256k1/building_block/). */
#define BPP_BLS12_381_G1 0
#define BPP_SECP256K1 1
/* edwards25519 (the curve under Ristretto255), prime-order subgroup, points as affine Edwards (x, y), L = 4.
 * The reference has NO such backend (only a stale README example): parity unpinned, see csrc/ed25519.hpp. */
#define BPP_ED25519 2

#define BPP_OK 0
#define BPP_VERIFICATION_ERROR 1
#define BPP_FORMAT_ERROR 2  /* ProofError::FormatError (src/errors.rs:20): per-proof status of the serialized-proof path */
#define BPP_E_ARG (-1)      /* bad argument (null pointer, unknown curve, n*m not a power of two...) */
#define BPP_E_HIP (-2)      /* HIP runtime error or another runtime failure inside the library; bpp_last_error() has the text */
#define BPP_E_LENGTH (-3)   /* "mulvec: lengths of scalars and points must match" and friends */
#define BPP_E_POINT (-4)    /* a point is not on the curve / coordinate >= p */
#define BPP_E_NOMEM (-5)

typedef struct bpp_ctx bpp_ctx;
typedef struct bpp_verifier bpp_verifier;

/* Arith::init (src/bls12_381/building_block/arith.rs:6-19): one-time library/device initialisation.
 * `device` is the HIP device ordinal. */
int bpp_init(int curve_id, int device, bpp_ctx **out_ctx);
void bpp_destroy(bpp_ctx *ctx);
const char *bpp_last_error(void);

/* words (uint64_t) per wire point for a curve: 2*L + 1 */
int bpp_point_words(int curve_id);

/* MulVec::calculate (src/bls12_381/building_block/mulvec.rs:20-33; secp256k1 twin
 * src/secp256k1/building_block/secp256k1/util.rs:22-36): out = sum_i scalars[i] * points[i].
 * n == 0 gives the point at infinity (Point::zero()).  Host pointers. */
int bpp_msm(bpp_ctx *ctx, const uint64_t *scalars, const uint64_t *points, size_t n, uint64_t *out);

/* The same MulVec through the bucket (Pippenger) pipeline regardless of n (bpp_msm switches to it by
 * itself from n = 4096 up); window_bits in [2, 16], 0 = chosen from n.  Host pointers. */
int bpp_msm_pippenger(bpp_ctx *ctx, const uint64_t *scalars, const uint64_t *points, size_t n, int window_bits,
                      uint64_t *out);

/* MulVec::calculate (mulvec.rs:20-33) with EVERY buffer in HBM, asynchronous on `stream` (a hipStream_t; NULL = default
 * stream): nothing is copied, nothing synchronises -- the seam for callers whose scalars and points already live on
 * the device, and what bench.py's `msm` leg times.  The bucket (Pippenger) pipeline of csrc/pippenger.hpp at any n:
 * signed c-bit windows with an unsigned top window, on BLS12-381 after the GLV split of every scalar (two 128-bit halves
 * per point), counting sort per window, one lane per bucket with an LDS-DMA gather ring, bucket sums reduced per tile
 * of 64 S buckets by one wave (running sums per lane, suffix scan and butterfly across the wave by shuffles).
 *   d_scalars : n scalars (4 x u64, canonical; values >= r are reduced on the device)
 *   d_points  : n wire points
 *   d_out     : one wire point (affine, canonical) -- the sum, bit for bit what bpp_msm returns
 *   d_status  : one uint32_t (may be NULL): 0, or 1 when some point was not on the curve / had a coordinate >= p (the
 *               host-pointer calls report BPP_E_POINT; here the point counts as infinity and the flag is raised)
 *   d_workspace: bpp_msm_workspace_bytes(ctx, n, window_bits) bytes
 * window_bits in [2, 16], 0 = chosen from n.  n == 0 gives Point::zero(). */
size_t bpp_msm_workspace_bytes(bpp_ctx *ctx, size_t n, int window_bits);
int bpp_msm_device(bpp_ctx *ctx, const uint64_t *d_scalars, const uint64_t *d_points, size_t n, int window_bits,
                   uint64_t *d_out, uint32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream);

/* Per-stage timing of bpp_msm_device with HIP events recorded on the caller's stream (stages: 0 sort = points from
 * wire, digits + histogram, scans, scatter; 1 bucket sums, chunk by chunk [dominant: k_pip_chunks]; 2 fold of the
 * segments into buckets; 3 bucket reduction per tile and per window; 4 doublings + final sum + affine point).
 * bpp_msm_profile averages over the calls recorded since profiling was switched on (at most 16): out_stage_ms[5];
 * out_shape (may be NULL) receives the geometry of the last call: n, items, windows, narrow window bits, wide
 * windows, buckets, entries per chunk, requested window bits. */
int bpp_msm_set_profiling(bpp_ctx *ctx, int on);
int bpp_msm_profile(bpp_ctx *ctx, float *out_stage_ms, size_t *out_passes, uint32_t *out_shape);

/* `count` independent MulVecs in one launch: MulVec c has lens[c] terms starting at offset
 * sum(lens[0..c)).  out: count points.  (The fold of src/weighted_inner_product_proof.rs:151-163 is
 * 2 n' MulVecs of length 2.)  Host pointers. */
int bpp_msm_batch(bpp_ctx *ctx, const uint64_t *scalars, const uint64_t *points, const uint32_t *lens,
                  size_t count, uint64_t *out);

/* Point * PrimeFieldElem for n independent pairs (src/bls12_381/building_block/point/point.rs:69-85).
 * Host pointers. */
int bpp_scalar_mul_batch(bpp_ctx *ctx, const uint64_t *scalars, const uint64_t *points, size_t n,
                         uint64_t *out);

/* PublicKey::new(length) (src/publickey.rs:21-48): g = base point, h = 2g, G_i = 3(i+1) g,
 * H_i = 5(i+1) g.  out_gh: 2 points [g, h]; out_G, out_H: `length` points each. */
int bpp_pk_new(bpp_ctx *ctx, size_t length, uint64_t *out_gh, uint64_t *out_G, uint64_t *out_H);

/* The production counterpart of PublicKey::new: g = the base point, h, G_i, H_i hashed to the group from `label`
 * (csrc/hash_to_group.hpp), so that no discrete-log relation between the generators is known.  The reference only has
 * the test generators above (its own comment at src/publickey.rs:23-39).  Not a standard hash-to-curve suite: try-and-
 * increment (+ cofactor clearing on BLS12-381 G1) for the Weierstrass curves, RFC 9496 element derivation for
 * ristretto255.  PARITY UNPINNED; restated in oracle/pyref.py. */
int bpp_pk_hashed(bpp_ctx *ctx, const uint8_t *label, size_t label_len, size_t length, uint64_t *out_gh,
                  uint64_t *out_G, uint64_t *out_H);

/* RangeProver::commit / PublicKey::commitment (src/range/prover.rs:28-42, src/publickey.rs:50-52):
 * out = g * new(v as i32) + h * gamma.  The `v as i32` truncation of prover.rs:37 is kept. */
int bpp_commit(bpp_ctx *ctx, const uint64_t *gh, uint64_t v, const uint64_t *gamma, uint64_t *out);
/* (bpp_commit_batch / bpp_commit_batch_device, below the mixed prove calls: `count` commitments over an engine's g and h
 * through its window tables, with or without the truncation.) */

/* RangeProof::prove (src/range/mod.rs:31-55 -> prove_single :80-187 / prove_multiple :240-403, and
 * WeightedInnerProductProof::prove, src/weighted_inner_product_proof.rs:36-227).
 * pk = (gh, G, H) with n*m generators each; v[m], gamma[m] (scalars), V[m] commitments.
 * out_points : 3 + 2k points  [A, wip.A, wip.B, L_0..L_{k-1}, R_0..R_{k-1}],  k = log2(n*m)
 * out_scalars: 3 scalars      [r', s', delta']
 * The proof is a function of (v, gamma, V): V is read, not formed.  A key that has been seen before proves through its
 * cached engine when V is what the batched prover forms from (v, gamma) -- the reference's new(v as i32) g + gamma h
 * (src/range/prover.rs:37) or, tried second, the untruncated v g + gamma h a caller brings for an amount of 2^31 or more
 * (BPP_PROVE_AMOUNT64 below) -- and through the fold-based prover for any other V; the output is the same either way. */
int bpp_range_prove(bpp_ctx *ctx, const uint64_t *gh, const uint64_t *G, const uint64_t *H, size_t n,
                    size_t m, const uint64_t *v, const uint64_t *gamma, const uint64_t *V,
                    uint64_t *out_points, uint64_t *out_scalars);

/* One folding round of WeightedInnerProductProof::prove as a seam of its own (src/weighted_inner_product_proof.rs:147-164),
 * in place on the first n' = len / 2 entries of each array (host pointers; a, b: len scalars; G, H: len points):
 *   a[i] = a[i] e + a[n'+i] y^n' e^-1 ;  b[i] = b[i] e^-1 + b[n'+i] e ;
 *   G[i] = MulVec[e^-1, y^-n' e].[G[i], G[n'+i]] ;  H[i] = MulVec[e, e^-1].[H[i], H[n'+i]]
 * y_nhat = y^n' (wip.rs:98), e = the round's challenge (wip.rs:131).  bpp_range_prove runs this per round on resident
 * vectors; the batched prover (bpp_range_prove_batch) never folds points at all (csrc/prover_batch.hpp). */
int bpp_wip_fold_round(bpp_ctx *ctx, uint64_t *a, uint64_t *b, uint64_t *G, uint64_t *H, size_t len,
                       const uint64_t *y_nhat, const uint64_t *e);

/* RangeProof::verify (src/range/mod.rs:57-78 -> verify_single :189-238 + wip verify
 * src/weighted_inner_product_proof.rs:238-328, or verify_multiple :405-510).
 * proof_points as written by bpp_range_prove with k rounds.  Returns 0 / 1 / negative.
 * The reference takes the public key with every call and pays the whole naive MulVec each time; so does the FIRST call
 * here with a given key (data-parallel naive MulVec, no setup).  When the same key comes back the context builds a
 * verifier with narrow window tables for it (c = 8: milliseconds to build, < 1 GB at n m = 1024) and that and later
 * calls run the batch verifier's pass at count = 1.  A cached entry is found by hash and confirmed by comparing the
 * key bytes; at most four keys, least recently used out; bpp_set_verify_cache(ctx, 0) switches the mechanism off and
 * frees it.  Points outside the prime-order group are judged by the full-curve sum, as the reference does: on BLS12-381
 * the cached verifier runs with the subgroup check on (bpp_verifier_set_subgroup_check), and a reject of the cached pass
 * is decided again by the table-free full-curve MulVec -- so a curve point outside G1 whose contribution cancels is
 * accepted, one whose contribution does not is rejected.  Verdicts do not depend on which path ran
 * (tests/test_gpu_verdict_parity.py). */
int bpp_set_verify_cache(bpp_ctx *ctx, int on);
int bpp_range_verify(bpp_ctx *ctx, const uint64_t *gh, const uint64_t *G, const uint64_t *H, size_t n,
                     size_t m, const uint64_t *proof_points, size_t k, const uint64_t *proof_scalars,
                     const uint64_t *V);

/* ---- batch verifier: the north-star path -----------------------------------------------------
 * A verifier holds the public key in HBM together with the fixed-base window tables built from it
 * (see DESIGN.md), for one (n, m).  Proof batches are DEVICE buffers (e.g. torch CUDA tensors'
 * data_ptr()), so a step of the hot path touches no host memory:
 *   d_points  : count x (3 + 2k + m) wire points   [A, wip.A, wip.B, L_0.., R_0.., V_0..V_{m-1}]
 *   d_scalars : count x 3 scalars                  [r', s', delta']
 *   d_ok      : count x uint32_t                   0 = Ok(()), 1 = Err(VerificationError)
 * The reference has no batch API (src/lib.rs:11-13); each entry of d_ok is exactly the verdict
 * RangeProof::verify would return for that proof.
 * window_bits in [2, 20] trades HBM for arithmetic: a b-bit scalar costs floor((b-1)/c) + 1 table additions per
 * generator and the tables hold about (2mn + 2) x b/c x 2^(c-1) affine points (n=64, m=16 on BLS12-381:
 * 7.0 GB at c = 13, 49.5 GB at c = 16, 215 GB at c = 17: BLS12-381 keeps one table for both halves of the endomorphism
 * split and returns BPP_E_ARG for a generator outside the prime-order subgroup).  BPP_E_NOMEM (-5) if they do not fit. */
int bpp_verifier_create(bpp_ctx *ctx, const uint64_t *gh, const uint64_t *G, const uint64_t *H, size_t n,
                        size_t m, int window_bits, bpp_verifier **out);
void bpp_verifier_destroy(bpp_verifier *v);
/* bytes of device workspace bpp_verifier_run needs for `count` proofs */
size_t bpp_verifier_workspace_bytes(const bpp_verifier *v, size_t count);
/* number of MulVec terms per proof, N = 2mn + 2k + m + 5 */
size_t bpp_verifier_msm_len(const bpp_verifier *v);
/* bytes of HBM held by the window tables */
size_t bpp_verifier_table_bytes(const bpp_verifier *v);

/* One pass of the hot path over a resident batch, asynchronous on `stream` (a hipStream_t; NULL =
 * default stream).  d_challenges is NULL (the reference's hard-coded "transcript") or
 * count x (3 + k) scalars [y, z, e, e_1..e_k] per proof.  Any 256-bit words are taken: a value >= r stands for its
 * residue mod r.  For a challenge that is 0 mod r the inverse the scalars call for (y^-1, e^-1 for m > 1, e_t^-1) is
 * taken as 0 -- no honest transcript yields one; the proof is judged by the scalars that follow from that -- and the
 * other proofs of the batch are unaffected.
 * Optional debug / parity outputs (NULL to skip):
 *   d_out_scalars: count x N scalars -- the MulVec scalars in the reference's MulVec order
 *                  (range/mod.rs:481-490 for m > 1, wip.rs:298-307 for m == 1)
 *   d_out_result : count x wire point -- the MulVec result ("expected", range/mod.rs:503)
 * The call only enqueues work on `stream` (kernels, and for a batch small enough to be latency bound an event fork/join
 * with a side stream of the verifier): after one eager call it can be captured into a HIP graph and replayed
 * (tests/test_gpu_round2.py::test_verifier_run_is_graph_capturable).
 * A verifier may be used by several host threads and on several streams at once, each pass with a workspace and a verdict
 * buffer of its own (the tables are read-only); the stage profiling is the exception: one thread while it is on.
 * Points are elements of the prime-order group (what the prover, mcl, or the decoder with its subgroup check produce).
 * On BLS12-381 the proof-carried points are multiplied through G1's endomorphism (GLV, as mcl itself does): for points
 * of G1 the result is sum s_i P_i bit for bit; a curve point OUTSIDE G1 is still processed deterministically and its
 * proof judged by the same equation, but the result point is then not the full-curve sum. */
int bpp_verifier_run(bpp_verifier *v, const uint64_t *d_points, const uint64_t *d_scalars, size_t count,
                     const uint64_t *d_challenges, uint32_t *d_ok, void *d_workspace,
                     size_t workspace_bytes, uint64_t *d_out_scalars, uint64_t *d_out_result,
                     void *stream);
/* ---- mixed batches: proofs of several aggregation sizes against ONE verifier's tables ----
 * A verifier created for (n, m) -- its "capacity" -- also verifies batches in which proof i has m_i commitments, m_i a
 * power of two <= m.  Proof i's verdict is RangeProof::verify(proof_i, PublicKey::new(n m_i), n, V_i)
 * (src/range/mod.rs:57-78, :189-238, :405-510): the verdict against the PREFIX key of the proof's own shape, i.e. the
 * first n m_i generators of the verifier's G and H vectors with its g and h (PublicKey::new(L) is a prefix of every
 * longer key, src/publickey.rs:21-48; so is bpp_pk_hashed(label, .), which derives each generator from its index).  No
 * table memory beyond the verifier's own is used: the tables of (n, m) hold every generator a shape (n, m_i) needs.
 *   m_of        : HOST array of count values m_i (the caller has parsed the proofs)
 *   d_points    : proof i's record [A, wip.A, wip.B, L.., R.., V_0..V_{m_i-1}] (3 + 2 k_i + m_i wire points,
 *                 k_i = log2(n m_i)) at wire point sum_{j<i} (3 + 2 k_j + m_j): packed, in caller order
 *   d_scalars   : count x 3 scalars [r', s', delta']
 *   d_challenges: NULL (the reference's literals for each proof's own shape) or 3 + k_i scalars [y, z, e, e_1..e_k]
 *                 per proof, packed in caller order
 *   d_ok        : count x uint32_t in caller order, 0 = Ok(()) / 1 = Err(VerificationError)
 *   d_out_result: NULL or count x wire point, the MulVec result of each proof, in caller order
 *   d_workspace : bpp_verifier_mixed_workspace_bytes(v, m_of, count) bytes (0 when an m_i is not taken)
 * An m_i that is zero, not a power of two or larger than m, a workspace that is too small or a NULL pointer returns
 * BPP_E_ARG, with the offending proof's index in bpp_last_error(), and enqueues nothing; count = 0 is BPP_OK.
 * The call BLOCKS the host while it uploads the per-proof index array (32 bytes per proof, a pageable copy on `stream`,
 * which first waits for the work already queued there); everything else is enqueued asynchronously on `stream`: the
 * gather of the records into one region per m_i (k_mixed_gather), one pass of bpp_verifier_run per m_i present over its
 * region, the verdicts back into caller order (k_mixed_scatter).  bpp_verifier_set_subgroup_check applies as it does to
 * bpp_verifier_run.  Several host threads may use one verifier at once, each call with a workspace and buffers of its
 * own, as for bpp_verifier_run. */
size_t bpp_verifier_mixed_workspace_bytes(const bpp_verifier *v, const uint32_t *m_of, size_t count);
int bpp_verifier_run_mixed(bpp_verifier *v, const uint64_t *d_points, const uint64_t *d_scalars, const uint32_t *m_of,
                           size_t count, const uint64_t *d_challenges, uint32_t *d_ok, void *d_workspace,
                           size_t workspace_bytes, uint64_t *d_out_result, void *stream);
/* Fiat-Shamir challenges of a mixed batch (see bpp_verifier_derive_challenges): proof i's transcript starts from the
 * prefix key of its own shape (n, m_i), as its prover's does.  d_challenges: 3 + k_i scalars per proof, packed in caller
 * order -- the layout bpp_verifier_run_mixed takes.  Arguments, errors and blocking as for bpp_verifier_run_mixed. */
int bpp_verifier_derive_challenges_mixed(bpp_verifier *v, const uint64_t *d_points, const uint32_t *m_of, size_t count,
                                         uint64_t *d_challenges, void *d_workspace, size_t workspace_bytes, void *stream);
/* bpp_verifier_run_mixed on HOST buffers (points, scalars, m_of laid out as above), the reference's literal challenges;
 * synchronous.  out_ok: count x uint32_t. */
int bpp_range_verify_batch_mixed(bpp_verifier *v, const uint64_t *points, const uint64_t *scalars, const uint32_t *m_of,
                                 size_t count, uint32_t *out_ok);

/* The same pass captured ONCE into a HIP graph and replayed: a small batch is a chain of a dozen launches and a stream
 * fork/join that a replay submits in one call.  bpp_verifier_graph_capture runs the pass once eagerly (argument checks;
 * what a pass creates lazily must exist before a capture), captures it on a stream of its own and instantiates the graph;
 * the device pointers and `count` are baked in: the caller refreshes the CONTENTS of d_points / d_scalars / d_challenges
 * between replays and reads d_ok after them.  bpp_graph_launch only enqueues (hipGraphLaunch on `stream`).  The verifier must
 * outlive its graphs; stage profiling must be off while capturing. */
typedef struct bpp_graph bpp_graph;
int bpp_verifier_graph_capture(bpp_verifier *v, const uint64_t *d_points, const uint64_t *d_scalars, size_t count,
                               const uint64_t *d_challenges, uint32_t *d_ok, void *d_workspace, size_t workspace_bytes,
                               bpp_graph **out);
int bpp_graph_launch(bpp_graph *g, void *stream);
void bpp_graph_destroy(bpp_graph *g);

/* RangeProof::prove for `count` independent provers that share (pk, n, m) -- and RangeProver::commit for
 * their values -- in one device-resident pass (csrc/prover_batch.hpp): the folding rounds of
 * src/weighted_inner_product_proof.rs:79-172 fold only scalars, every L, R, A, B is a MulVec over the
 * original generators through the engine's window tables.  Output is bit-identical to bpp_range_prove.
 *   v: count x m uint64_t ; gamma: count x m scalars
 *   out_points : count x (3 + 2k) points [A, wip.A, wip.B, L.., R..] ; out_scalars: count x 3 scalars
 *   out_V      : count x m commitments (may be NULL).  Host pointers. */
int bpp_range_prove_batch(bpp_verifier *engine, const uint64_t *v, const uint64_t *gamma, size_t count,
                          uint64_t *out_points, uint64_t *out_scalars, uint64_t *out_V);

/* The same pass with every buffer in HBM (what bench.py's `prove` leg times): d_v count x m uint64_t, d_gamma
 * count x m scalars, outputs as above (d_out_V may be NULL), asynchronous on `stream`; no host memory is touched
 * and nothing synchronises.  The batch is processed in chunks that reuse d_workspace
 * (bpp_prover_workspace_bytes(engine, count) bytes). */
size_t bpp_prover_workspace_bytes(const bpp_verifier *engine, size_t count);
int bpp_range_prove_batch_device(bpp_verifier *engine, const uint64_t *d_v, const uint64_t *d_gamma, size_t count,
                                 uint64_t *d_out_points, uint64_t *d_out_scalars, uint64_t *d_out_V,
                                 void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- combined batch check ("final multiscalar check") -- an engine mode, NOT a reference code path ----
 * One random linear combination of the batch's verification MulVecs, sum_p w_p * M_p == identity, with 128-bit
 * weights w_p (csrc/combined.hpp): the fixed generators collapse to one fixed-base MulVec, the proof-carried
 * points run through the verifier's Straus kernels and are summed window by window.  An all-valid batch always
 * passes.  A batch holding an invalid proof fails except with probability ~2^-128 -- PROVIDED the weights could not
 * be predicted by whoever made the proofs; with a fixed or guessable key two invalid proofs can be made to cancel.
 * So the weights come from the caller, one of
 *   d_weights  : count x 16 bytes on the device (little-endian 128-bit values), e.g. from a transcript over the
 *                whole batch; or
 *   weight_key : 32 secret bytes (host pointer) from the OS CSPRNG, fresh per call or per verifier; the device
 *                expands w_p = SHA-256(key || "bppw" || (index_base + p) as u64)[0..16).  index_base is the GLOBAL index
 *                of this call's first proof, so ranks that share a key never share a weight.  The 16 bytes are read
 *                little-endian and 0 stands for 1 (d_weights likewise); index_base + p past 2^64 is left unspecified.
 * The caller falls back to bpp_verifier_run for the exact per-proof verdicts of the reference when the check fails.
 * It assumes proof points of the prime-order subgroup (bpp_proofs_decode checks that for serialized proofs).
 *   d_out_partial: bpp_verifier_partial_bytes() bytes -- this call's weighted sum (opaque jacobian image) followed by
 *                  a validity word (non-zero when a proof of this call carried an invalid point); ranks exchange
 *                  these once (RCCL all-gather) and bpp_verifier_sum_partials adds the sums and ORs the words
 *   d_ok         : one uint32_t, 0 iff the partial is the identity and every proof point was valid */
size_t bpp_verifier_partial_bytes(const bpp_verifier *v);
size_t bpp_verifier_combined_workspace_bytes(const bpp_verifier *v, size_t count);
int bpp_verifier_run_combined(bpp_verifier *v, const uint64_t *d_points, const uint64_t *d_scalars, size_t count,
                              const uint64_t *d_challenges, const uint8_t *weight_key, uint64_t index_base,
                              const uint64_t *d_weights, void *d_out_partial, uint32_t *d_ok, void *d_workspace,
                              size_t workspace_bytes, void *stream);
/* d_partials: n partials of bpp_verifier_partial_bytes() bytes each; d_ok = 0 iff their sum is the identity and no
 * rank reported an invalid point */
int bpp_verifier_sum_partials(bpp_verifier *v, const void *d_partials, size_t n, uint32_t *d_ok, void *stream);

/* ---- grouped check -- per-proof verdicts at (nearly) the combined check's price; an engine mode, NOT a reference path ----
 * The reference verifies one proof at a time (src/range/mod.rs:57-78).  A service that needs the verdict of EVERY proof
 * but expects nearly all of them to be valid does not have to pay the per-proof MulVec: neighbouring proofs are checked
 * in groups of `group` (a power of two >= 2; 32 is a good default), sum_{p in group} w_p * M_p == identity, each group as
 * ONE virtual proof of the batch verifier's last stages, and only the proofs of a group that fails go through the exact
 * per-proof path (bpp_verifier_run) afterwards.  Weights, their key and index_base as for bpp_verifier_run_combined, and
 * the same conditions: a group holding an invalid proof passes with probability ~2^-128 if the weights were unpredictable
 * and the proof points lie in the prime-order subgroup (bpp_verifier_set_subgroup_check / the serialized path).
 *   d_out_verdicts : count x uint32_t, 0 = Ok / 1 = VerificationError -- the vector bpp_verifier_run writes
 *   stats          : HOST pointer, may be NULL: [groups that failed, proofs re-verified exactly]
 * The call synchronises `stream` (the list of failing groups comes back to the host between the two passes), so it
 * cannot be captured into a graph. */
size_t bpp_verifier_grouped_workspace_bytes(const bpp_verifier *v, size_t count, uint32_t group);
int bpp_verifier_run_grouped(bpp_verifier *v, const uint64_t *d_points, const uint64_t *d_scalars, size_t count,
                             const uint64_t *d_challenges, const uint8_t *weight_key, uint64_t index_base,
                             const uint64_t *d_weights, uint32_t group, uint32_t *d_out_verdicts, uint64_t *stats,
                             void *d_workspace, size_t workspace_bytes, void *stream);

/* The same in two calls, so that ONE host thread can keep several batches in flight (a stream, a workspace and a verdict
 * buffer per batch): bpp_verifier_grouped_begin only enqueues the weighted checks of the groups; bpp_verifier_grouped_finish,
 * given the same buffers, count, group and stream, synchronises that stream, reads the groups' verdicts and re-verifies the
 * proofs of the failing ones.  begin(A), begin(B), finish(A), begin(C), finish(B), ... hides the latency-bound parts of one
 * batch behind the other (+13 % on (64,16) x 8192).  bpp_verifier_run_grouped = begin + finish. */
int bpp_verifier_grouped_begin(bpp_verifier *v, const uint64_t *d_points, const uint64_t *d_scalars, size_t count,
                               const uint64_t *d_challenges, const uint8_t *weight_key, uint64_t index_base,
                               const uint64_t *d_weights, uint32_t group, uint32_t *d_out_verdicts, void *d_workspace,
                               size_t workspace_bytes, void *stream);
int bpp_verifier_grouped_finish(bpp_verifier *v, const uint64_t *d_points, const uint64_t *d_scalars, size_t count,
                                const uint64_t *d_challenges, uint32_t group, uint32_t *d_out_verdicts, uint64_t *stats,
                                void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- Fiat-Shamir transcript (csrc/transcript.hpp) -- what the reference's constants stand in for --------
 * The reference has no transcript (every challenge is a literal, src/range/mod.rs:278-279,
 * :417-418, src/weighted_inner_product_proof.rs:131, :211, :353, :369; the intended labels survive as a comment at
 * src/weighted_inner_product_proof.rs:339-348).  PARITY UNPINNED: pinned by oracle/pyref.py and the C oracle.
 * bpp_verifier_derive_challenges hashes each proof record of a resident batch (SHA-256, one lane per proof) into the
 * block [y, z, e, e_1..e_k] that bpp_verifier_run / bpp_verifier_run_combined accept as d_challenges:
 *   d_points     : count x (3 + 2k + m) wire points, as for bpp_verifier_run
 *   d_challenges : count x (3 + k) scalars (out)
 * bpp_range_prove_batch_fs is the prover under the same transcript (round t + 1 waits for L_t, R_t); outputs as
 * bpp_range_prove_batch_device.  An infinity enters the transcript as its canonical image (zero coordinates, flag = 1)
 * whatever non-zero flag word the caller wrote: one byte string per group element. */
int bpp_verifier_derive_challenges(bpp_verifier *v, const uint64_t *d_points, size_t count, uint64_t *d_challenges,
                                   void *stream);
/* Blinding.  The reference's blinding values are literals (alpha = 7 / 33, range/mod.rs:94,256; d_L = 4, d_R = 5,
 * wip.rs:94-95; r, s, delta, eta = 33, 44, 88, 123, wip.rs:175-178), so a proof made with them is sound but NOT hiding:
 * with those known, r', s', delta' give away the folded a, b and a linear combination of the gammas (for m = 1: gamma
 * itself, hence v).  That is kept, bit for bit, in the reference-parity calls (bpp_range_prove, bpp_range_prove_batch*).
 * Under the transcript the caller supplies the blinding: per proof alpha, r, s, delta, eta and d_L[t], d_R[t] for each of
 * the k rounds, one of
 *   d_blinding : count x (5 + 2k) canonical scalars on the device [alpha, r, s, delta, eta, d_L[0..k), d_R[0..k)]; or
 *   blind_key  : 32 secret bytes (host pointer) from the OS CSPRNG; the device expands slot j of proof p as
 *                (c0 + 2^256 c1) mod r, c_h = SHA-256(key || "bppb" || (index_base + p) as u64 LE || j as u32 LE || h as
 *                u32 LE) read little-endian (zero -> one).  index_base is the GLOBAL index of this call's first proof: a
 *                key must never meet the same index twice.
 * Both NULL: the literals above (for parity tests against the oracle's transcript-mode prover; such proofs leak).
 * host buffers, as bpp_range_prove_batch */
int bpp_range_prove_batch_fs(bpp_verifier *engine, const uint64_t *v, const uint64_t *gamma, size_t count,
                             const uint8_t *blind_key, uint64_t index_base, uint64_t *out_points, uint64_t *out_scalars,
                             uint64_t *out_V);
/* device buffers, as bpp_range_prove_batch_device; d_out_challenges: count x (3 + k) scalars [y, z, e, e_1..e_k] the
 * prover drew (may be NULL) */
int bpp_range_prove_batch_fs_device(bpp_verifier *engine, const uint64_t *d_v, const uint64_t *d_gamma, size_t count,
                                    const uint8_t *blind_key, uint64_t index_base, const uint64_t *d_blinding,
                                    uint64_t *d_out_points, uint64_t *d_out_scalars, uint64_t *d_out_V,
                                    uint64_t *d_out_challenges, void *d_workspace, size_t workspace_bytes, void *stream);

/* Points of unknown origin.  bpp_verifier_run takes wire points that are elements of the prime-order group by
 * construction (what the prover, mcl, or the decoders with their subgroup check produce), and on BLS12-381 evaluates the
 * proof-carried points through G1's endomorphism: for a curve point OUTSIDE G1 the MulVec is then not the full-curve sum
 * (on the order-3 point T = (0, 2) the engine forms (k1 - k2) T where the definition gives (k1 + k2 z^2) T), so a proof
 * whose R_0 was replaced by R_0 + T is ACCEPTED by the raw call where a full-curve evaluation rejects it
 * (tests/test_gpu_round3.py pins both outcomes).  on != 0 makes every wire point of a pass go through the membership
 * test of the decoders (csrc/ec.hpp aff_in_prime_subgroup; two multiplications by |z| per point, about +20 % on a (64,16)
 * pass); a point outside the group then counts as an invalid point and its proof gets verdict 1.  Off by default.  A
 * no-op on secp256k1 (cofactor 1); the edwards25519 instantiation works in ristretto255's quotient group instead: its
 * verdict test accepts a sum in E[4] (csrc/ristretto.hpp), i.e. points that differ by 4-torsion are THE SAME element
 * for every ed25519 entry point, raw wire points included -- the transcript hashes their ristretto255 encoding. */
int bpp_verifier_set_subgroup_check(bpp_verifier *v, int on);

/* Per-stage timing with HIP events recorded on the caller's stream around the kernels of a pass
 * (stages: 0 wire->Montgomery, 1 verifier scalars, 2 fixed-generator MSM [dominant; its first blocks also run
 * the Horner stage of the proof-point MSM], 3 proof-point MSM: digits, per-point tables, window sums,
 * 4 finalize).  The stages run back to back on one stream.  bpp_verifier_profile averages over the passes
 * recorded since profiling was switched on (at most 64): out_stage_ms[5]. */
int bpp_verifier_set_profiling(bpp_verifier *v, int on);
int bpp_verifier_profile(bpp_verifier *v, float *out_stage_ms, size_t *out_passes, unsigned *out_blocks_per_proof);

/* Host-pointer convenience over bpp_verifier_run (allocates, copies, synchronises). */
int bpp_range_verify_batch(bpp_verifier *v, const uint64_t *points, const uint64_t *scalars, size_t count,
                           uint32_t *out_ok);

/* ---- compressed point encodings: a data format next to the path ---------------------------------
 * The reference has no serialization; its commented-out size() functions (src/range/mod.rs:512-517,
 * src/weighted_inner_product_proof.rs:384-397) assume compressed points + 32-byte scalars and
 * src/errors.rs:20 reserves ProofError::FormatError for it.  PARITY UNPINNED by the reference; pinned by the
 * encodings' public generator vectors and oracle/pyref.py.
 *   BLS12-381 G1: 48 bytes, x big-endian, byte 0 bit 7 = compressed, bit 6 = infinity, bit 5 = y > (p-1)/2
 *   secp256k1   : 33 bytes, SEC1 02/03 || x big-endian; infinity = 33 zero bytes
 *   edwards25519: 32 bytes, ristretto255 (RFC 9496): the encoding of the prime-order quotient group, csrc/ristretto.hpp  Decompression runs on the device (one square root per point);
 * out_ok[i] = 0 valid, 1 malformed (flags, x >= p, x not on the curve) -- such a point is returned as infinity. */
size_t bpp_point_compressed_bytes(int curve_id);
int bpp_points_compress(bpp_ctx *ctx, const uint64_t *points, size_t n, uint8_t *out);
int bpp_points_decompress(bpp_ctx *ctx, const uint8_t *in, size_t n, uint64_t *out_points, uint32_t *out_ok);
/* device buffers, asynchronous on `stream`: feeds bpp_verifier_run's d_points without touching the host.
 * check_subgroup != 0: a curve point outside the prime-order subgroup is malformed too (BLS12-381 G1; what the container
 * decoder always does) */
int bpp_points_decompress_device(bpp_ctx *ctx, const void *d_in, size_t n, uint64_t *d_points, uint32_t *d_ok,
                                 int check_subgroup, void *stream);
/* bpp_range_verify_batch over serialized proofs: records = count x (3 + 2k + m) compressed points in the order
 * of d_points above, scalars = count x 3 (4 x u64 each).  out_ok[p] = 0 Ok / 1 VerificationError / 2 FormatError: a
 * malformed point encoding, a point outside the prime-order subgroup or a scalar >= the group order is a FormatError. */
int bpp_range_verify_batch_compressed(bpp_verifier *v, const uint8_t *records, const uint64_t *scalars, size_t count,
                                      uint32_t *out_ok);

/* ---- serialized proofs: the container -------------------------------------------------------------------
 * The reference never serializes a proof; its commented-out size() functions (src/range/mod.rs:512-517,
 * src/weighted_inner_product_proof.rs:384-397) count compressed points and 32-byte scalars, and src/errors.rs:20
 * reserves ProofError::FormatError for a deserializer.  PARITY UNPINNED; pinned by oracle/pyref.py's restatement.
 * One proof = bpp_proof_bytes(curve, n, m) bytes:
 *   "BPP+" | version = 1 | curve id | n | m | k = log2(n m) | 0 0 0            (12 bytes)
 *   A, wip.A, wip.B, L_0..L_{k-1}, R_0..R_{k-1}   compressed points (48 / 33 / 32 bytes each: BLS12-381 G1 ZCash form,
 *                                                 SEC1, ristretto255)
 *   r', s', delta'                                 32-byte little-endian scalars, canonical (< group order)
 * Decoding rejects with BPP_FORMAT_ERROR (2): a wrong header, a malformed point encoding, a point off the curve, a point
 * OUTSIDE THE PRIME-ORDER SUBGROUP (BLS12-381 G1 has a 126-bit cofactor: checked with the curve's endomorphism,
 * csrc/ec.hpp aff_in_prime_subgroup), a non-canonical scalar.  Host pointers. */
size_t bpp_proof_bytes(int curve_id, size_t n, size_t m);
int bpp_proofs_encode(bpp_ctx *ctx, size_t n, size_t m, const uint64_t *points, const uint64_t *scalars, size_t count,
                      uint8_t *out);
/* Container VERSION 2 (round 3): the same layout with UNCOMPRESSED points -- BLS12-381 G1 96 bytes (x | y big-endian, byte 0
 * bit 7 = 0, bit 6 = infinity, bit 5 = 0), secp256k1 SEC1 0x04 | x | y (65 bytes; infinity = 65 zero bytes); not offered
 * for ristretto255.  Decoding then needs no square root (a third of the decoder's arithmetic: 7.6 -> 5.4 ms per 8 192
 * (64,16) proofs) for 48 / 32 more bytes per point; every other check is the same (header with version = 2, coordinates
 * < p, on the curve, in the prime-order subgroup, canonical scalars).  The verify entry points take it with
 * BPP_SER_UNCOMPRESSED, and then expect the commitments uncompressed too (bpp_points_uncompressed). */
size_t bpp_point_uncompressed_bytes(int curve_id);
int bpp_points_uncompressed(bpp_ctx *ctx, const uint64_t *points, size_t n, uint8_t *out);
size_t bpp_proof_bytes_version(int curve_id, size_t n, size_t m, int version);
int bpp_proofs_encode_version(bpp_ctx *ctx, size_t n, size_t m, int version, const uint64_t *points, const uint64_t *scalars,
                              size_t count, uint8_t *out);
/* out_points: count x (3 + 2k) wire points (infinity where an encoding was rejected); out_status: 0 / BPP_FORMAT_ERROR.
 * Reads version 1 containers (a version 2 header is a FormatError here: those are consumed by the verify entry points). */
int bpp_proofs_decode(bpp_ctx *ctx, size_t n, size_t m, const uint8_t *in, size_t count, uint64_t *out_points,
                      uint64_t *out_scalars, uint32_t *out_status);
/* RangeProof::verify for `count` serialized proofs: proofs count x bpp_proof_bytes, commitments count x m compressed
 * points.  flags: BPP_SER_TRANSCRIPT (1): challenges from the Fiat-Shamir transcript instead of the reference's
 * constants; BPP_SER_UNCOMPRESSED (2): container version 2, proofs count x bpp_proof_bytes_version(.., 2) and the
 * commitments count x m uncompressed points.  out_ok[p] = 0 Ok / 1 VerificationError / 2 FormatError. */
#define BPP_SER_TRANSCRIPT 1
#define BPP_SER_UNCOMPRESSED 2
int bpp_range_verify_batch_serialized(bpp_verifier *v, const uint8_t *proofs, const uint8_t *commitments, size_t count,
                                      int flags, uint32_t *out_ok);
/* The same with every buffer in HBM, asynchronous on `stream`, no host synchronisation: what a service that receives
 * proofs off the wire calls after one copy.  One kernel decodes the containers and the commitments (header, point
 * encodings with the subgroup check, scalar canonicity) straight into bpp_verifier_run's record layout inside the
 * workspace; d_ok[p] = 0 / 1 / 2 as above.  d_workspace: bpp_verifier_serialized_workspace_bytes(v, count) bytes. */
size_t bpp_verifier_serialized_workspace_bytes(const bpp_verifier *v, size_t count);
int bpp_range_verify_batch_serialized_device(bpp_verifier *v, const void *d_proofs, const void *d_commitments, size_t count,
                                             int flags, uint32_t *d_ok, void *d_workspace, size_t workspace_bytes,
                                             void *stream);
/* ... and with the grouped check (above) behind the decoder: the same status vector (0 / 1 / 2 per proof) at the grouped
 * check's price when the batch is (nearly) all valid.  weight_key: 32 fresh secret bytes (host); index_base, group, stats as
 * for bpp_verifier_run_grouped; the decoder's subgroup check provides the prime-order points the weighted check assumes.
 * Synchronises `stream`.  d_workspace: bpp_verifier_serialized_grouped_workspace_bytes(v, count, group) bytes. */
size_t bpp_verifier_serialized_grouped_workspace_bytes(const bpp_verifier *v, size_t count, uint32_t group);
int bpp_range_verify_batch_serialized_grouped_device(bpp_verifier *v, const void *d_proofs, const void *d_commitments,
                                                     size_t count, int flags, const uint8_t *weight_key, uint64_t index_base,
                                                     uint32_t group, uint32_t *d_ok, uint64_t *stats, void *d_workspace,
                                                     size_t workspace_bytes, void *stream);

/* ---- serialized proofs of MIXED aggregation sizes: a block of bytes off the wire against ONE verifier's tables ----
 * bpp_range_verify_batch_serialized_device for a batch in which proof i carries m_i commitments, m_i a power of two <=
 * the verifier's m (see "mixed batches" above).  d_ok[i], in caller order, is 0 Ok / 1 VerificationError / 2 FormatError,
 * the verdict being RangeProof::verify(proof_i, PublicKey::new(n m_i), n, V_i): the prefix key of the proof's own shape,
 * exactly as bpp_verifier_run_mixed defines it; FormatError takes precedence as on the single-shape path.
 *   d_proofs      : the containers packed back to back in caller order, container i of
 *                   bpp_proof_bytes_version(curve, n, m_of[i], version) bytes
 *   d_commitments : m_of[i] encoded commitments per proof, packed in caller order
 *   m_of          : HOST array of count values m_i (the framing layer knows each length; bpp_proofs_scan recovers them
 *                   from a bare stream)
 *   flags         : BPP_SER_TRANSCRIPT, BPP_SER_UNCOMPRESSED as above (version 2 is refused for ristretto255)
 *   d_workspace   : bpp_verifier_serialized_mixed_workspace_bytes(v, m_of, count) bytes (0 when an m_i is not taken)
 * A container whose header disagrees with m_of[i] (m, k, n, curve, version, magic, reserved bytes) is a FormatError OF
 * THAT PROOF ONLY: every length comes from m_of, never from the bytes, so its neighbours are read where they are.
 * An m_i that is zero, not a power of two or larger than m, a workspace that is too small or a NULL pointer returns
 * BPP_E_ARG, with the offending proof's index in bpp_last_error(), enqueues nothing and leaves d_ok untouched; so does a
 * batch of 4 GiB or more of containers or of commitments (the per-proof index holds 32-bit byte offsets); count = 0 is
 * BPP_OK.
 * The call BLOCKS the host while it uploads the per-proof index array (16 bytes per proof, a pageable copy on `stream`,
 * which first waits for the work already queued there); everything else is enqueued asynchronously on `stream`: one
 * decode of every container straight into one region of records per m_i (k_container_decode_mixed; no record is copied a
 * second time), the subgroup test, per m_i present the challenges (BPP_SER_TRANSCRIPT) and one pass of bpp_verifier_run
 * over its region, the statuses back into caller order.  bpp_verifier_set_subgroup_check applies as it does to
 * bpp_range_verify_batch_serialized_device.  Several host threads may use one verifier at once, each call with a
 * workspace and buffers of its own. */
size_t bpp_verifier_serialized_mixed_workspace_bytes(const bpp_verifier *v, const uint32_t *m_of, size_t count);
int bpp_range_verify_batch_serialized_mixed_device(bpp_verifier *v, const void *d_proofs, const void *d_commitments,
                                                   const uint32_t *m_of, size_t count, int flags, uint32_t *d_ok,
                                                   void *d_workspace, size_t workspace_bytes, void *stream);
/* the same on HOST buffers (proofs, commitments, m_of laid out as above); synchronous.  out_ok: count x uint32_t. */
int bpp_range_verify_batch_serialized_mixed(bpp_verifier *v, const uint8_t *proofs, const uint8_t *commitments,
                                            const uint32_t *m_of, size_t count, int flags, uint32_t *out_ok);
/* ---- the grouped check over MIXED batches: wire records (bpp_verifier_run_mixed's input) and bytes off the wire ----
 * bpp_verifier_run_grouped's verdicts for a batch in which proof i has m_of[i] commitments: the vector bpp_verifier_run_mixed
 * writes (each proof against the prefix key of its own shape), at the grouped check's price when (nearly) every proof is
 * valid, from ONE verifier's tables.  Input layout, m_of rules and blocking as for bpp_verifier_run_mixed; weights
 * (weight_key / index_base / d_weights), group, stats, the verdict words, the soundness conditions and the stream
 * synchronisation as for bpp_verifier_run_grouped.
 * THE PARTITION.  The batch is gathered by aggregation size: all proofs with m_i = 1 in caller order, then those with
 * m_i = 2, 4, ...  Group g holds the gathered positions [g * group, min(count, (g + 1) * group)): a group may hold proofs of
 * two or more sizes and the last one may be short.  The partition depends on (m_of, group) only, so it is fixed before a
 * weight is drawn; stats = [groups that failed, proofs re-verified exactly] follows from it and the exact verdicts.
 * THE WEIGHTS belong to the caller's numbering: proof i (caller order) is weighted with PRF(weight_key, index_base + i), or
 * with d_weights[i] (count x 16 bytes, caller order).
 * Each group is one virtual proof of the verifier's CAPACITY shape (the generators of a smaller shape are generators of the
 * capacity tables), so the last stages run once for the whole batch; a group costs one capacity-sized fixed-generator
 * MulVec whatever the sizes of its proofs.
 * Errors: BPP_E_ARG for an m_of[i] that is not taken (the text names i), a group that is not a power of two >= 2, a
 * workspace that is too small, a NULL pointer; nothing is enqueued or written then.  count = 0 is BPP_OK, stats = {0, 0}.
 * The workspace-size calls return 0 for an m_of or a group that is not taken. */
size_t bpp_verifier_grouped_mixed_workspace_bytes(const bpp_verifier *v, const uint32_t *m_of, size_t count, uint32_t group);
int bpp_verifier_run_grouped_mixed(bpp_verifier *v, const uint64_t *d_points, const uint64_t *d_scalars, const uint32_t *m_of,
                                   size_t count, const uint64_t *d_challenges, const uint8_t *weight_key, uint64_t index_base,
                                   const uint64_t *d_weights, uint32_t group, uint32_t *d_out_verdicts, uint64_t *stats,
                                   void *d_workspace, size_t workspace_bytes, void *stream);
/* ... behind the decoder: bpp_range_verify_batch_serialized_mixed_device's status vector (0 / 1 / 2 in caller order; both
 * container versions, BPP_SER_TRANSCRIPT) through the grouped check above.  weight_key is required.  A container the decoder
 * rejects keeps FormatError whatever its group did, changes no other proof's status, and counts its group as failed. */
size_t bpp_verifier_serialized_grouped_mixed_workspace_bytes(const bpp_verifier *v, const uint32_t *m_of, size_t count,
                                                             uint32_t group);
int bpp_range_verify_batch_serialized_grouped_mixed_device(bpp_verifier *v, const void *d_proofs, const void *d_commitments,
                                                           const uint32_t *m_of, size_t count, int flags,
                                                           const uint8_t *weight_key, uint64_t index_base, uint32_t group,
                                                           uint32_t *d_ok, uint64_t *stats, void *d_workspace,
                                                           size_t workspace_bytes, void *stream);

/* ---- PROVING blocks of mixed aggregation sizes with one engine: the producing side of the mixed verify calls ----
 * One engine created for capacity (n, m) proves a block in which proof i has m_of[i] values, m_of[i] a power of two <= m
 * (the rules and error texts of bpp_verifier_run_mixed).  Proof i is, bit for bit, RangeProof::prove (reference
 * src/range/mod.rs:31-55, :80-187, :240-403; src/weighted_inner_product_proof.rs:36-227; commitments
 * src/range/prover.rs:28-42) for PublicKey::new(n m_i), the prefix key of its own shape: what bpp_range_prove_batch* gives
 * on a dedicated (n, m_i) engine of the same key.  The output is written once, straight into the layout the mixed verifier
 * reads.
 *   d_v, d_gamma     : sum m_i uint64_t / sum m_i scalars, packed in caller order (device)
 *   m_of             : HOST array of count values m_i
 *   flags            : 0: the reference's literal challenges and blinding.  BPP_SER_TRANSCRIPT: Fiat-Shamir, as
 *                      bpp_range_prove_batch_fs_device, with blinding from blind_key (32 bytes, host), or from d_blinding
 *                      (5 + 2 k_i scalars per proof, packed in caller order, device), or -- both NULL -- the literals.
 *                      Blinding without BPP_SER_TRANSCRIPT is BPP_E_ARG.
 *                      BPP_PROVE_AMOUNT64 (0x100, defined below; alone or with the above): full 64-bit amounts.
 *                      The reference forms a commitment as new(v as i32) g + gamma h (src/range/prover.rs:37) while the witness bits come from
 *                      the whole u64, so its proof of an amount of 2^31 or more does not verify; with this flag the scalar
 *                      on g is the uint64_t itself (below r on every curve).  Nothing else changes -- bits of a_L,
 *                      challenges, blinding, layout -- and for v < 2^31 the output is bit-identical with and without it.
 *                      With n < 64 and v >= 2^n the call succeeds and the proof does not verify, as out of range
 *                      values behave without the flag.
 *   index_base       : the blinding index belongs to the CALLER's numbering: proof i uses index_base + i whatever its
 *                      place inside the engine (the rule bpp_verifier_run_grouped_mixed states for its weights)
 *   d_out_points     : proof i's record [A, wip.A, wip.B, L.., R.., V_0..V_{m_i-1}] at wire point
 *                      sum_{j<i} (3 + 2 k_j + m_j): exactly bpp_verifier_run_mixed's d_points
 *   d_out_scalars    : count x 3 scalars [r', s', delta'], caller order
 *   d_out_challenges : NULL, or the packed 3 + k_i blocks [y, z, e, e_1..e_k]: bpp_verifier_run_mixed's d_challenges
 *   d_workspace      : bpp_prover_mixed_workspace_bytes(engine, m_of, count) bytes (0 when an m_i is not taken)
 * Errors: BPP_E_ARG for an m_of[i] that is not taken (the text names i), a NULL pointer, a workspace that is too small,
 * blind_key and d_blinding both given, an unknown flag; nothing is enqueued and no output is written then.  count = 0 is
 * BPP_OK.  The call BLOCKS the host only while it uploads the per-proof index (a pageable copy on `stream`); everything else
 * is enqueued asynchronously on `stream`: per m_i present a gather of its values and gammas and bpp_range_prove_batch*'s
 * kernels over the prefix view of the tables, the records written through the index (k_pb_collect). */
#define BPP_PROVE_AMOUNT64 0x100
size_t bpp_prover_mixed_workspace_bytes(const bpp_verifier *engine, const uint32_t *m_of, size_t count);
int bpp_range_prove_batch_mixed_device(bpp_verifier *engine, const uint64_t *d_v, const uint64_t *d_gamma, const uint32_t *m_of,
                                       size_t count, int flags, const uint8_t *blind_key, uint64_t index_base,
                                       const uint64_t *d_blinding, uint64_t *d_out_points, uint64_t *d_out_scalars,
                                       uint64_t *d_out_challenges, void *d_workspace, size_t workspace_bytes, void *stream);
/* The same proofs as BYTES (reference: as above; the container has no reference counterpart, see "serialized proofs"):
 * container i of bpp_proof_bytes_version(curve, n, m_of[i], version) bytes, packed back to back in caller order in
 * d_out_proofs, and m_of[i] encoded commitments per proof packed in d_out_commitments -- the input of
 * bpp_range_verify_batch_serialized_mixed_device, and a stream bpp_proofs_scan frames.  flags also takes
 * BPP_SER_UNCOMPRESSED (container version 2, commitments uncompressed; BPP_E_ARG on ristretto255) and BPP_PROVE_AMOUNT64
 * (the untruncated commitment scalar in place of src/range/prover.rs:37's `v as i32`, as above).  The 4 GiB limits of
 * the 32-bit byte index apply as on the verify side.  The records are proved into workspace regions per m_i and one kernel
 * (k_container_encode_mixed) writes every byte of the two output buffers.  Errors and blocking as above. */
size_t bpp_prover_serialized_mixed_workspace_bytes(const bpp_verifier *engine, const uint32_t *m_of, size_t count);
int bpp_range_prove_batch_serialized_mixed_device(bpp_verifier *engine, const uint64_t *d_v, const uint64_t *d_gamma,
                                                  const uint32_t *m_of, size_t count, int flags, const uint8_t *blind_key,
                                                  uint64_t index_base, const uint64_t *d_blinding, void *d_out_proofs,
                                                  void *d_out_commitments, void *d_workspace, size_t workspace_bytes,
                                                  void *stream);
/* Both on HOST buffers (RangeProof::prove per proof, src/range/mod.rs:31-55), synchronous; layouts as above, blinding from
 * blind_key or the literals.  out_challenges may be NULL.  flags as above, BPP_PROVE_AMOUNT64 (src/range/prover.rs:37
 * without its truncation) included. */
int bpp_range_prove_batch_mixed(bpp_verifier *engine, const uint64_t *v, const uint64_t *gamma, const uint32_t *m_of,
                                size_t count, int flags, const uint8_t *blind_key, uint64_t index_base, uint64_t *out_points,
                                uint64_t *out_scalars, uint64_t *out_challenges);
int bpp_range_prove_batch_serialized_mixed(bpp_verifier *engine, const uint64_t *v, const uint64_t *gamma, const uint32_t *m_of,
                                           size_t count, int flags, const uint8_t *blind_key, uint64_t index_base,
                                           uint8_t *out_proofs, uint8_t *out_commitments);

/* ---- commitments for a block of amounts through the engine's tables ----
 * RangeProver::commit (reference src/range/prover.rs:28-42) for `count` values over the engine's g and h:
 *     out_V[i] = s_i g + gamma_i h,   s_i = new(v_i as i32) with flags = 0 (the truncation of src/range/prover.rs:37, so
 *     each point equals bpp_commit's), s_i = v_i, the whole uint64_t, with BPP_PROVE_AMOUNT64.
 * One lane per commitment walks the window-table rows of g and h (k_commit_batch, csrc/commit.hpp): a table gather and a
 * mixed addition per non-zero digit, no doubling; a 64-bit amount has at most ceil(65 / window_bits) non-zero digits.
 *   d_v, d_gamma : count uint64_t / count scalars (device); gamma is read as bpp_range_prove_batch_mixed_device reads it
 *                  (canonical, < r)
 *   d_out_V      : count wire points in caller order, in the form the prover writes its commitments (the same image of
 *                  the point at infinity; on ristretto255 the same representative)
 * The device call only enqueues on `stream`: no workspace, no host synchronisation.  The host call copies around it and
 * reduces gamma mod r first, as the host prove calls do.  BPP_E_ARG for a NULL pointer or any other flag bit, nothing
 * written; count = 0 is BPP_OK. */
int bpp_commit_batch_device(bpp_verifier *engine, const uint64_t *d_v, const uint64_t *d_gamma, size_t count, int flags,
                            uint64_t *d_out_V, void *stream);
int bpp_commit_batch(bpp_verifier *engine, const uint64_t *v, const uint64_t *gamma, size_t count, int flags,
                     uint64_t *out_V);

/* ---- mask recovery ("rewind") and scanning: the receiver's side of a proof ----
 * "Blinding" above states as a warning that whoever knows alpha, delta, eta, d_L, d_R reads a linear combination of the
 * gammas off delta'.  For the holder of the blinding key that is the feature: the key derives exactly those scalars from
 * (blind_key, index, slot), so the mask of an output comes back out of its proof.  The quantities inverted are the
 * prover's own (reference src/range/mod.rs:159-172: alpha_hat = alpha + y^(nm+1) gamma, the m > 1 form at :366-376;
 * src/weighted_inner_product_proof.rs:94-95,175-227: d_L, d_R enter alpha in every round, delta' = eta + delta e +
 * alpha e^2).  With [y, z, e, e_1..e_k] the challenge block of a proof of shape (n, m), k = log2(n m):
 *     alpha_k = (delta' - eta - delta e) e^-2
 *     S       = (alpha_k - sum_t (e_t^2 d_L[t] + e_t^-2 d_R[t]) - alpha) y^-(nm+1)
 *     Gamma   = gamma_0 + z^2 gamma_1 + .. + z^(2(m-1)) gamma_{m-1}  =  S for m = 1, S z^-2 for m > 1
 * so for a single output Gamma IS its mask gamma.  A zero challenge leaves an inversion undefined: Gamma is then written
 * as zero (and a scan treats the proof as unconfirmed).
 * A SCAN IS NOT A VERIFICATION.  Nothing here checks a proof: Gamma of an invalid proof is a number like any other, and
 * status 0 below says that V_0 opens to (v, Gamma), not that the proof is sound.  Scan what has been verified.
 * blind_key TOGETHER WITH THE INDEX IS A VIEW KEY for every proof made with it: whoever holds both reads the mask of
 * every single-output proof the key blinded (and Gamma of the aggregated ones).  Hand it out as such, to wallets and
 * auditors, and to nobody else.  THE INDEX RULE HOLDS: a key never meets an index twice, on the proving side; the recovery
 * must name the index each proof was MADE with, in the caller's numbering -- d_index[i] when given, else index_base + i.  A
 * scanner does not see proofs in the order they were made: d_index carries that order.
 * The blinding source is one of: blind_key (32 bytes, host) with the index rule above; d_blinding (device), the prover's
 * layout, 5 + 2 k_i canonical scalars per proof packed in caller order; both NULL, the reference's literals (whose proofs
 * hide nothing).  m_of follows "mixed batches" above (HOST array, m_i a power of two <= the engine's m).
 * A proof is sixteen lanes of k_recover_masks (csrc/recover.hpp), one per term; every shape bpp_verifier_create admits has
 * at most 14 terms (k <= 12), and a k above 14 would be BPP_E_ARG.
 *
 * RECOVERY FROM WIRE DATA reads the scalar triples and the challenge blocks only, no points:
 *   d_scalars     : count x 3 scalars [r', s', delta'] in caller order (bpp_verifier_run_mixed's)
 *   d_challenges  : the packed 3 + k_i blocks (bpp_verifier_derive_challenges_mixed's output), or NULL: the literals of
 *                   each proof's own shape
 *   d_out_masks   : count x 4 words, canonical Gamma_i in caller order
 *   d_workspace   : bpp_recover_mixed_workspace_bytes(v, m_of, count) bytes (0 when an m_i is not taken)
 * SCANNING FROM BYTES takes bpp_range_verify_batch_serialized_mixed_device's input (d_proofs, d_commitments, m_of) and
 * runs its decoder, membership test and -- BPP_SER_TRANSCRIPT -- challenges, then the recovery instead of the verifier's
 * pass, and for single outputs the confirmation V_0 == v g + Gamma h through the engine's window tables
 * (k_recover_confirm, the lane of k_commit_batch).
 *   flags         : BPP_SER_TRANSCRIPT | BPP_SER_UNCOMPRESSED | BPP_PROVE_AMOUNT64 (the scalar on g is the whole uint64_t,
 *                   as the proofs were made; without it new(v as i32), src/range/prover.rs:37)
 *   d_amounts     : count x uint64_t, one candidate amount per proof in caller order, read for m_i = 1 only; may be NULL
 *   d_out_masks   : count x 4 words ; d_status : count words, caller order:
 *                     0                     m_i = 1, amount given, V_0 == v g + Gamma h: the output belongs to the key and
 *                                           Gamma is its mask
 *                     1                     m_i = 1, amount given, the equation fails (another key, another amount); mask zero
 *                     2                     the decoder's FormatError, exactly as in the verify calls; mask zero
 *                     BPP_SCAN_UNCONFIRMED  no amount given, or m_i > 1: Gamma is written as computed
 *   d_workspace   : bpp_scan_serialized_mixed_workspace_bytes(v, m_of, count) bytes (0 when an m_i is not taken)
 * Errors: BPP_E_ARG for a NULL required pointer, a workspace that is too small, an m_of[i] that is not taken (the text
 * names i), blind_key and d_blinding both given, d_index without blind_key, blinding without BPP_SER_TRANSCRIPT on the
 * scan calls (as the prove calls rule), an unknown flag; nothing is enqueued and nothing is written then.  count = 0 is
 * BPP_OK.  Both device calls BLOCK the host only while they upload the per-proof index; the rest is enqueued on `stream`.
 * The host-buffer twins take every buffer (index, blinding, amounts included) from the host and are synchronous. */
#define BPP_SCAN_UNCONFIRMED 3
size_t bpp_recover_mixed_workspace_bytes(const bpp_verifier *v, const uint32_t *m_of, size_t count);
int bpp_range_recover_masks_mixed_device(bpp_verifier *v, const uint64_t *d_scalars, const uint32_t *m_of, size_t count,
                                         const uint64_t *d_challenges, const uint8_t *blind_key, uint64_t index_base,
                                         const uint64_t *d_index, const uint64_t *d_blinding, uint64_t *d_out_masks,
                                         void *d_workspace, size_t workspace_bytes, void *stream);
int bpp_range_recover_masks_mixed(bpp_verifier *v, const uint64_t *scalars, const uint32_t *m_of, size_t count,
                                  const uint64_t *challenges, const uint8_t *blind_key, uint64_t index_base,
                                  const uint64_t *index, const uint64_t *blinding, uint64_t *out_masks);
size_t bpp_scan_serialized_mixed_workspace_bytes(const bpp_verifier *v, const uint32_t *m_of, size_t count);
int bpp_range_scan_serialized_mixed_device(bpp_verifier *v, const void *d_proofs, const void *d_commitments,
                                           const uint32_t *m_of, size_t count, int flags, const uint8_t *blind_key,
                                           uint64_t index_base, const uint64_t *d_index, const uint64_t *d_blinding,
                                           const uint64_t *d_amounts, uint64_t *d_out_masks, uint32_t *d_status,
                                           void *d_workspace, size_t workspace_bytes, void *stream);
int bpp_range_scan_serialized_mixed(bpp_verifier *v, const uint8_t *proofs, const uint8_t *commitments, const uint32_t *m_of,
                                    size_t count, int flags, const uint8_t *blind_key, uint64_t index_base,
                                    const uint64_t *index, const uint64_t *blinding, const uint64_t *amounts,
                                    uint64_t *out_masks, uint32_t *out_status);

/* ---- scanning a block under MANY keys: bpp_range_scan_serialized_mixed* for n_keys view keys in one call ----
 * A wallet server, an exchange or an auditor tests every block against all the keys it holds.  Most of a scan does not
 * depend on the key -- the container decode, the membership test, the challenges, the k + 1 inversions per proof -- so
 * this call does that once and spends per (key, proof) pair only the 2k + 3 slot expansions and as many products: Gamma
 * is affine in the blinding slots, Gamma = A0 + sum_s c_s slot_s(key, index) with public coefficients (c_alpha = -D,
 * c_delta = -D e^-1, c_eta = -D e^-2, c_dL[t] = -D e_t^2, c_dR[t] = -D e_t^-2, c_r = c_s = 0, A0 = D e^-2 delta',
 * D = (y^(nm+1) [z^2])^-1; csrc/recover_coeffs.hpp).  Every pair gets exactly the status and mask
 * bpp_range_scan_serialized_mixed gives for that key.
 * EVERY KEY HERE TOGETHER WITH THE INDEX IS A VIEW KEY, as stated above for blind_key: whoever holds both reads the mask
 * of every single-output proof the key blinded.  A SCAN IS NOT A VERIFICATION.  The device call reads the keys from the
 * caller's buffer into registers and copies them nowhere: nothing derived from a key but Gamma reaches memory.  The host
 * twin uploads the keys into a buffer of its own and overwrites that buffer before freeing it, on every return path.
 *   d_proofs, d_commitments, m_of, count : as bpp_range_scan_serialized_mixed_device takes them
 *   flags         : BPP_SER_TRANSCRIPT (REQUIRED: keys are the only blinding source here) | BPP_SER_UNCOMPRESSED |
 *                   BPP_PROVE_AMOUNT64, each meaning what it means there
 *   d_keys        : n_keys x 32 bytes (device, 4-byte aligned), key j at d_keys + 32 j
 *   index_base, d_index : the blinding index of proof i, SHARED BY ALL KEYS: d_index[i] (count x uint64_t, device) when
 *                   given, else index_base + i
 *   d_amounts     : KEY-MAJOR n_keys x count uint64_t, d_amounts[j * count + i] the candidate amount of proof i under key
 *                   j, read for m_i = 1 only; may be NULL
 *   d_out_masks   : KEY-MAJOR n_keys x count x 4 words; d_status : KEY-MAJOR n_keys x count words -- pair (j, i) at
 *                   j * count + i, 36 bytes of output per pair; the status words are those of the single-key call (2, the
 *                   decoder's FormatError, under every key)
 *   d_workspace   : bpp_scan_serialized_mixed_keys_workspace_bytes(v, m_of, count, n_keys) bytes (0 when an m_i is not
 *                   taken or n_keys x count is over the bound)
 * Errors: BPP_E_ARG for a NULL required pointer, a d_keys that is not 4-byte aligned, flags without BPP_SER_TRANSCRIPT, an
 * unknown flag, an m_of[i] that is not taken (the text names i), n_keys x count above 0x7fffffff / 64 (checked without
 * overflow), a workspace that is too small; nothing is enqueued and nothing is written then.  n_keys = 0 or count = 0 is
 * BPP_OK.  The device call BLOCKS the host only while it uploads the per-proof index; the host twin is synchronous. */
size_t bpp_scan_serialized_mixed_keys_workspace_bytes(const bpp_verifier *v, const uint32_t *m_of, size_t count,
                                                      size_t n_keys);
int bpp_range_scan_serialized_mixed_keys_device(bpp_verifier *v, const void *d_proofs, const void *d_commitments,
                                                const uint32_t *m_of, size_t count, int flags, const uint8_t *d_keys,
                                                size_t n_keys, uint64_t index_base, const uint64_t *d_index,
                                                const uint64_t *d_amounts, uint64_t *d_out_masks, uint32_t *d_status,
                                                void *d_workspace, size_t workspace_bytes, void *stream);
int bpp_range_scan_serialized_mixed_keys(bpp_verifier *v, const uint8_t *proofs, const uint8_t *commitments,
                                         const uint32_t *m_of, size_t count, int flags, const uint8_t *keys, size_t n_keys,
                                         uint64_t index_base, const uint64_t *index, const uint64_t *amounts,
                                         uint64_t *out_masks, uint32_t *out_status);

/* ---- sealed amounts: the 8-byte ciphertext of its amount that an output carries ----
 * A scanner has no candidate amount per (key, proof) pair; a real output carries ONE ciphertext of its amount and every
 * view key tries its own pad on it:
 *     pad(key, idx) = the first 8 bytes, read as a little-endian uint64_t, of
 *                     SHA-256(key || "bppa" || idx as u64 LE || 0 as u32 || 0 as u32)
 *     sealed        = amount XOR pad(key, idx)
 * the 52-byte block of the blinding slots under the tag "bppa" in place of "bppb": domain-separated from every scalar
 * that enters a proof (csrc/find_terms.hpp).  Sealing and opening are the same operation.  idx is the blinding index of
 * the output's proof and THE INDEX RULE ABOVE HOLDS UNCHANGED: output i has index d_index[i] when given, else
 * index_base + i, and a key never meets an index twice.  The pad hides an amount from whoever lacks the key; it does not
 * authenticate it -- what ties an opened amount to an output is the confirmation V_0 == v g + Gamma h of the call below.
 *   blind_key : 32 bytes (HOST); it travels to the kernel by value and is stored nowhere
 *   d_in, d_out : count x uint64_t (device); may be the same buffer
 * Errors: BPP_E_ARG for a NULL ctx, blind_key, d_in or d_out and a count above 0x7fffffff / 64; count = 0 is BPP_OK.
 * Asynchronous on `stream`; the host twin takes host buffers and is synchronous. */
int bpp_amounts_seal_device(bpp_ctx *ctx, const uint8_t *blind_key, uint64_t index_base, const uint64_t *d_index,
                            const uint64_t *d_in, size_t count, uint64_t *d_out, void *stream);
int bpp_amounts_seal(bpp_ctx *ctx, const uint8_t *blind_key, uint64_t index_base, const uint64_t *index, const uint64_t *in,
                     size_t count, uint64_t *out);

/* ---- VERIFY a block and LIST the outputs of many view keys in one call ----
 * What a scanning service wants of a block: one verdict per proof and the short list of outputs that belong to its keys.
 * With the calls above that is bpp_range_verify_batch_serialized_mixed_device, then
 * bpp_range_scan_serialized_mixed_keys_device on what passed, then a walk over 36 bytes per (key, proof) pair.  This call
 * runs their common front (index upload, container decode, membership test, challenges) ONCE, then today's exact pass
 * per class, then for the single outputs the many-key scan's pair kernels, the confirmation and a compaction.
 * THIS CALL IS A VERIFICATION OF THE BLOCK: d_ok[i] is exactly the word bpp_range_verify_batch_serialized_mixed_device
 * writes for the same bytes and flags -- 0 Ok / 1 VerificationError / 2 FormatError -- for every proof, aggregated ones
 * included.  A HIT is a pair (key j, proof i) with
 *     m_i = 1,  d_ok[i] == 0,  no zero challenge (the coefficients of Gamma are defined),  V_0 == v g + Gamma h
 * where Gamma is the mask recovered under key j and v the candidate amount of the pair.  A HIT IMPLIES A VERIFIED PROOF:
 * a proof that opens under its owner's key but fails verification (a tampered r', say) is status 0 in the scan calls and
 * is NOT a hit here.  Aggregated proofs (m_i > 1) are verified and never listed.
 * EVERY KEY HERE TOGETHER WITH THE INDEX IS A VIEW KEY, as stated above.  The device call reads the keys from the
 * caller's buffer into registers and copies them nowhere: nothing derived from a key but Gamma, and for a hit its
 * amount, reaches memory, and no Gamma of a pair that is not a hit is left in the workspace when the call's kernels
 * have run.  The host twin uploads the keys into a buffer of its own and overwrites that buffer before freeing it, on
 * every return path.
 *   d_proofs, d_commitments, m_of, count, d_keys, n_keys, index_base, d_index :
 *                   as bpp_range_scan_serialized_mixed_keys_device takes them
 *   flags         : BPP_SER_TRANSCRIPT (REQUIRED) | BPP_SER_UNCOMPRESSED | BPP_PROVE_AMOUNT64, each meaning what it means
 *                   there, | BPP_FIND_AMOUNTS_SEALED
 *   d_amounts     : REQUIRED (nothing could be confirmed without it).  With BPP_FIND_AMOUNTS_SEALED: count x uint64_t
 *                   sealed amounts in caller order, SHARED BY ALL KEYS -- the candidate of pair (j, i) is
 *                   d_amounts[i] XOR pad(key_j, index_i), formed in registers.  Without it: the KEY-MAJOR
 *                   n_keys x count array of the many-key scan.  Read for m_i = 1 only.
 *   d_ok          : count words, caller order, as above
 *   d_hits        : max_hits records of 12 words: [key number j, caller position i, amount lo, amount hi, Gamma as 8
 *                   canonical words], IN ASCENDING (key number, caller position) ORDER, the same from run to run
 *   d_n_hits      : one word: the number of hits FOUND.  When it exceeds max_hits only the first max_hits records in that
 *                   order are written; nothing beyond min(n_hits, max_hits) records is touched, and the caller sees the
 *                   overflow from the count.  d_hits may be NULL when max_hits = 0.
 *   d_workspace   : bpp_verify_find_serialized_mixed_keys_workspace_bytes(v, m_of, count, n_keys) bytes (0 when an m_i is
 *                   not taken or n_keys x count is over the bound); it grows with n_keys: 44 bytes per pair
 * Nothing else is written: no dense status matrix, no dense mask matrix.
 * Errors: BPP_E_ARG for a NULL required pointer (d_ok and d_n_hits among them; with n_keys > 0 also d_keys, d_amounts, and
 * d_hits when max_hits > 0), a
 * d_keys that is not 4-byte aligned, flags without BPP_SER_TRANSCRIPT, an unknown flag, an m_of[i] that is not taken (the
 * text names i), n_keys x count above 0x7fffffff / 64 (checked without overflow), a workspace that is too small; nothing
 * is enqueued and nothing is written then.  count = 0 is BPP_OK with d_n_hits[0] = 0 and nothing else written.
 * n_keys = 0 is BPP_OK with d_n_hits[0] = 0 too, AND THE BLOCK IS VERIFIED ALL THE SAME: d_ok is written as above (the
 * pass needs no key; d_keys, d_amounts and d_hits are not read and may be NULL), so d_ok never comes back unwritten from
 * a successful call with count > 0.  The device call BLOCKS the host only while it uploads the per-proof index; the host
 * twin is synchronous and writes min(n_hits, max_hits) records. */
#define BPP_FIND_AMOUNTS_SEALED 0x200
size_t bpp_verify_find_serialized_mixed_keys_workspace_bytes(const bpp_verifier *v, const uint32_t *m_of, size_t count,
                                                             size_t n_keys);
int bpp_range_verify_find_serialized_mixed_keys_device(bpp_verifier *v, const void *d_proofs, const void *d_commitments,
                                                       const uint32_t *m_of, size_t count, int flags, const uint8_t *d_keys,
                                                       size_t n_keys, uint64_t index_base, const uint64_t *d_index,
                                                       const uint64_t *d_amounts, uint32_t *d_ok, uint32_t *d_hits,
                                                       size_t max_hits, uint32_t *d_n_hits, void *d_workspace,
                                                       size_t workspace_bytes, void *stream);
int bpp_range_verify_find_serialized_mixed_keys(bpp_verifier *v, const uint8_t *proofs, const uint8_t *commitments,
                                                const uint32_t *m_of, size_t count, int flags, const uint8_t *keys,
                                                size_t n_keys, uint64_t index_base, const uint64_t *index,
                                                const uint64_t *amounts, uint32_t *out_ok, uint32_t *out_hits, size_t max_hits,
                                                uint32_t *out_n_hits);

/* ---- view tags: the one byte an output carries so that a scanner can rule out foreign keys cheaply ----
 * The find call above pays 2k + 3 slot expansions, as many products in Fr and a table walk for EVERY (key, output) pair,
 * and a service with hundreds of keys owns almost none of a block's outputs.  A tagged output carries one byte more:
 *     view_tag(key, idx) = the first byte of SHA-256(key || "bppt" || idx as u64 LE || 0 as u32 || 0 as u32)
 * the 52-byte block of the sealed amount's pad under a third domain tag (csrc/find_terms.hpp).  THE SENDER MAKES THE TAG,
 * under the recipient's key, next to the sealed amount; the scanner computes it first -- ONE compression per pair -- and
 * does the expensive work only where it matches: 255 of 256 foreign pairs stop there.  idx is the blinding index of the
 * output's proof and THE INDEX RULE ABOVE HOLDS UNCHANGED: d_index[i] when given, else index_base + i.
 * The tag hides nothing that a one-byte PRF output does not, and IT DOES NOT AUTHENTICATE ANYTHING: a wrong tag hides an
 * output from its owner's scan exactly as a wrong sealed amount does, and a matching tag proves nothing -- what ties an
 * output to a key is still the confirmation V_0 == v g + Gamma h.
 *   blind_key : 32 bytes (HOST); it travels to the kernel by value and is stored nowhere
 *   d_out     : count bytes (device)
 * Errors: BPP_E_ARG for a NULL ctx, blind_key or d_out and a count above 0x7fffffff / 64; count = 0 is BPP_OK.
 * Asynchronous on `stream`; the host twin takes host buffers and is synchronous. */
int bpp_view_tags_device(bpp_ctx *ctx, const uint8_t *blind_key, uint64_t index_base, const uint64_t *d_index, size_t count,
                         uint8_t *d_out, void *stream);
int bpp_view_tags(bpp_ctx *ctx, const uint8_t *blind_key, uint64_t index_base, const uint64_t *index, size_t count,
                  uint8_t *out);

/* ---- VERIFY a block and LIST the outputs of many view keys, TESTING THE VIEW TAGS FIRST ----
 * bpp_range_verify_find_serialized_mixed_keys_device with two more arguments; every other argument, every flag and every
 * rule stated there holds here, and that call is unchanged.  d_ok IS EXACTLY THE UNTAGGED CALL'S.  A CANDIDATE is a pair
 * (key j, proof i) with
 *     m_i = 1,  d_ok[i] == 0,  the decoder's status 0,  no zero challenge,  view_tag(key_j, index_i) == d_tags[i]
 * and A HIT IS A CANDIDATE THAT IS A HIT OF THE UNTAGGED CALL: the tag can only remove pairs.  Records, their order
 * (ascending key number, then caller position), max_hits and d_n_hits are as there.  The tag is independent of how
 * amounts are offered (sealed or key-major).
 *   d_tags         : count bytes, caller order, SHARED BY ALL KEYS, read for m_i = 1 only; REQUIRED when n_keys > 0
 *   d_n_candidates : one word, may be NULL: the pairs that passed the tag test (hits and chance matches of foreign keys)
 *   d_workspace    : bpp_verify_find_tagged_workspace_bytes(v, m_of, count, n_keys) bytes, a function of those alone with
 *                    room for every pair being a candidate; 0 where the untagged size function gives 0
 * Per pair the call computes one compression and moves one bit; slots are expanded and tables walked for candidates only.
 * The key rule, extended by one sentence: nothing derived from a key reaches memory but the candidate bit (the match of a
 * public byte), the hit bit, Gamma of a candidate (zeroed on a miss) and a hit's amount.
 * Errors: those of the untagged call, and BPP_E_ARG for a NULL d_tags with n_keys > 0; nothing is enqueued and nothing is
 * written then.  count = 0 is BPP_OK with d_n_hits[0] = 0, and d_n_candidates[0] = 0 when given; n_keys = 0 and a block of
 * nothing but aggregated proofs likewise, THE BLOCK VERIFIED ALL THE SAME (d_keys, d_amounts, d_tags, d_hits may be NULL).
 * The device call BLOCKS the host only while it uploads the per-proof index: the candidate count never travels to the
 * host.  The host twin is synchronous. */
size_t bpp_verify_find_tagged_workspace_bytes(const bpp_verifier *v, const uint32_t *m_of, size_t count, size_t n_keys);
int bpp_range_verify_find_tagged_serialized_mixed_keys_device(bpp_verifier *v, const void *d_proofs, const void *d_commitments,
                                                              const uint32_t *m_of, size_t count, int flags,
                                                              const uint8_t *d_keys, size_t n_keys, uint64_t index_base,
                                                              const uint64_t *d_index, const uint64_t *d_amounts, uint32_t *d_ok,
                                                              uint32_t *d_hits, size_t max_hits, uint32_t *d_n_hits,
                                                              const uint8_t *d_tags, uint32_t *d_n_candidates, void *d_workspace,
                                                              size_t workspace_bytes, void *stream);
int bpp_range_verify_find_tagged_serialized_mixed_keys(bpp_verifier *v, const uint8_t *proofs, const uint8_t *commitments,
                                                       const uint32_t *m_of, size_t count, int flags, const uint8_t *keys,
                                                       size_t n_keys, uint64_t index_base, const uint64_t *index,
                                                       const uint64_t *amounts, uint32_t *out_ok, uint32_t *out_hits,
                                                       size_t max_hits, uint32_t *out_n_hits, const uint8_t *tags,
                                                       uint32_t *out_n_candidates);

/* ---- outputs with DERIVED masks: finding each key's outputs INSIDE AGGREGATED PROOFS ----
 * The calls above list single-output proofs, by rewinding them.  A real transaction is ONE aggregated proof over two or
 * more outputs that belong to different people, and rewinding cannot serve it: an aggregated proof yields one
 * Gamma = sum z^(2j) gamma_j, never the individual gamma_j, and its nonces come from one blinding key.  So here nothing is
 * rewound.  The SENDER derives the mask of output j from the RECIPIENT's key and commits with it; the recipient derives it
 * again and checks the commitment.  With
 *     B(tag, idx, a, b) = SHA-256(key || tag (4 ASCII bytes) || idx as u64 LE || a as u32 LE || b as u32 LE)
 * the 52-byte block of the blinding slots, the pad and the view tag (csrc/output_terms.hpp):
 *     output_mask(key, idx, j) = (c0 + 2^256 c1) mod r, zero replaced by one; c_h = B("bppm", idx, j, h) read as a
 *                                little-endian 256-bit integer
 *     output_pad(key, idx, j)  = the first 8 bytes of B("bppa", idx, j, 0) as a little-endian uint64_t
 *     output_tag(key, idx, j)  = the first byte of B("bppt", idx, j, 0)
 * idx is the blinding index of the output's PROOF and THE INDEX RULE ABOVE HOLDS UNCHANGED: proof i has index d_index[i]
 * when given, else index_base + i, and a key never meets the same (idx, j) twice.  j is the output's place in that proof,
 * 0 <= j < m_i.  FOR j = 0 THE PAD AND THE TAG ARE BYTE FOR BYTE bpp_amounts_seal's pad AND bpp_view_tags's tag: a single
 * output sealed and tagged with those calls is a valid output here.  The mask's tag "bppm" separates it from every
 * blinding slot ("bppb"): the proof's own nonces stay the sender's business, under whatever key the sender proves.
 *
 * THE SENDER'S CALL, one lane per output:
 *   d_keys      : n_out x 32 bytes (device, 4-byte aligned): the recipient's key of each output
 *   d_index     : n_out x uint64_t: the blinding index of the output's proof
 *   d_j         : n_out x uint32_t: the output's place in its proof
 *   d_amounts   : n_out x uint64_t
 *   d_out_masks : n_out x 4 uint64_t words, canonical, in exactly the d_gamma layout that bpp_commit_batch_device and the
 *                 mixed prove calls read: they plug in without a copy
 *   d_out_sealed: n_out x uint64_t: amount XOR output_pad
 *   d_out_tags  : n_out bytes
 * Any of the three outputs may be NULL and is then skipped; all three NULL is BPP_E_ARG.  A MASK IS SECRET: whoever holds
 * it and the amount can open the commitment, and whoever holds (key, idx, j) holds the mask.  Errors: BPP_E_ARG for a
 * NULL ctx, a NULL input, a d_keys that is not 4-byte aligned, n_out above 0x7fffffff / 64; n_out = 0 is BPP_OK.
 * A proof over any number of outputs (the *_outs* calls below) needs no other form of this call: it is per output, with
 * j < outs_of[i], and a padded place has no output to make.
 * Asynchronous on `stream`, no workspace and no upload; the host twin takes host buffers, is synchronous and overwrites
 * its device copies of the keys and the masks before freeing them. */
int bpp_outputs_make_device(bpp_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_index, const uint32_t *d_j,
                            const uint64_t *d_amounts, size_t n_out, uint64_t *d_out_masks, uint64_t *d_out_sealed,
                            uint8_t *d_out_tags, void *stream);
int bpp_outputs_make(bpp_ctx *ctx, const uint8_t *keys, const uint64_t *index, const uint32_t *j, const uint64_t *amounts,
                     size_t n_out, uint64_t *out_masks, uint64_t *out_sealed, uint8_t *out_tags);

/* THE RECEIVER'S CALL: VERIFY a block and LIST, PER OUTPUT, what belongs to many view keys.  d_proofs, d_commitments, m_of,
 * count, d_keys, n_keys, index_base, d_index, d_ok, d_hits, max_hits, d_n_hits, d_n_candidates, d_workspace,
 * workspace_bytes and stream each mean what they mean in bpp_range_verify_find_tagged_serialized_mixed_keys_device.
 *   flags    : BPP_SER_TRANSCRIPT (REQUIRED) | BPP_SER_UNCOMPRESSED | BPP_PROVE_AMOUNT64.  BPP_FIND_AMOUNTS_SEALED is NOT
 *              accepted: amounts are always sealed here
 *   d_sealed : n_out x uint64_t, n_out = sum of m_i
 *   d_tags   : n_out bytes
 * Both are per OUTPUT, packed in caller order: output j of proof i is output number o = (sum of m_i' over i' < i) + j.
 * Both are SHARED BY ALL KEYS and REQUIRED when n_keys > 0.
 * d_ok IS WORD FOR WORD WHAT bpp_range_verify_batch_serialized_mixed_device WRITES.  A CANDIDATE is a pair (key q, output
 * o = (i, j)) with
 *     d_ok[i] == 0,  output_tag(key_q, idx_i, j) == d_tags[o]
 * and A HIT is a candidate with
 *     V_{i,j} == v g + gamma h,  v = d_sealed[o] XOR output_pad(key_q, idx_i, j),  gamma = output_mask(key_q, idx_i, j)
 * FOR EVERY m_i; the scalar on g is formed under the call's BPP_PROVE_AMOUNT64 as the commit calls form it.  A HIT IMPLIES
 * A VERIFIED PROOF.  Hit records are the 12 words of the calls above, [key number q, output number o, amount lo, amount
 * hi, gamma as 8 canonical words], IN ASCENDING (key number, output number) ORDER; max_hits and d_n_hits as there.
 * d_n_candidates (may be NULL) is the sum over the block.  The pair bound is n_keys x n_out <= 0x7fffffff / 64, checked
 * without overflow; bpp_verify_find_outputs_workspace_bytes(v, m_of, count, n_keys) is 0 beyond it and for an m_i that is
 * not taken.
 * THE KEY RULE, stronger here than above: no kernel of this call uses LDS or scratch, and nothing derived from a key
 * reaches memory except the candidate bit (the match of a public byte), the hit bit, and a HIT's gamma and amount.  A
 * non-hit's mask never leaves registers.  The host twin overwrites its copy of the keys before freeing it.
 * Errors: those of the tagged call (d_sealed in the place of d_amounts), and BPP_E_ARG for BPP_FIND_AMOUNTS_SEALED;
 * nothing is enqueued and nothing is written then.  count = 0 is BPP_OK with d_n_hits[0] = 0, and d_n_candidates[0] = 0
 * when given; n_keys = 0 likewise, THE BLOCK VERIFIED ALL THE SAME (d_keys, d_sealed, d_tags, d_hits may be NULL).  The
 * device call BLOCKS the host only while it uploads the per-proof index; the host twin is synchronous. */
size_t bpp_verify_find_outputs_workspace_bytes(const bpp_verifier *v, const uint32_t *m_of, size_t count, size_t n_keys);
int bpp_range_verify_find_outputs_serialized_mixed_keys_device(bpp_verifier *v, const void *d_proofs, const void *d_commitments,
                                                               const uint32_t *m_of, size_t count, int flags,
                                                               const uint8_t *d_keys, size_t n_keys, uint64_t index_base,
                                                               const uint64_t *d_index, const uint64_t *d_sealed,
                                                               const uint8_t *d_tags, uint32_t *d_ok, uint32_t *d_hits,
                                                               size_t max_hits, uint32_t *d_n_hits, uint32_t *d_n_candidates,
                                                               void *d_workspace, size_t workspace_bytes, void *stream);
int bpp_range_verify_find_outputs_serialized_mixed_keys(bpp_verifier *v, const uint8_t *proofs, const uint8_t *commitments,
                                                        const uint32_t *m_of, size_t count, int flags, const uint8_t *keys,
                                                        size_t n_keys, uint64_t index_base, const uint64_t *index,
                                                        const uint64_t *sealed, const uint8_t *tags, uint32_t *out_ok,
                                                        uint32_t *out_hits, size_t max_hits, uint32_t *out_n_hits,
                                                        uint32_t *out_n_candidates);

/* ---- proofs over ANY number of outputs (csrc/outs_plan.hpp) ----
 * Transactions have 2, 3, 5, 6 .. outputs; the argument needs a power of two.  A proof over o outputs, 1 <= o <= the
 * engine's m, IS the proof of shape (n, M), M = 2^ceil(log2 o), over the values v_0 .. v_{o-1}, 0, .., 0 and the masks
 * gamma_0 .. gamma_{o-1}, 0, .., 0: its commitments V_o .. V_{M-1} are the identity.  No new protocol:
 *   verdict    : RangeProof::verify(proof, PublicKey::new(n M), n, [V_0 .. V_{o-1}, identity x (M - o)]) -- exactly what
 *                bpp_range_verify_batch_serialized_mixed_device gives for m_of[i] = M when the caller appends the identity's
 *                encoding M - o times
 *   transcript : M points under "V" as ever, a padded one as the canonical infinity
 *   container  : byte for byte the container of shape (n, M); its header says m = M; bpp_proofs_scan returns M
 *   the count  : framing.  It travels as the host array outs_of[count], the way m_of does, and the value, mask and
 *                commitment streams carry outs_of[i] entries per proof, NOT M: sum of outs_of[i] in all, packed in caller order
 * The calls below are the serialized mixed calls with outs_of in the place of m_of; every other argument, flag, verdict
 * word and error is the one documented there.  The padded commitments are neither read nor decompressed nor tested for
 * group membership, a padded place is never paired with a key, and no byte of d_sealed / d_tags stands for it.
 * THE OUTPUT COUNT IS NOT AUTHENTICATED beyond this: a proof over [V_0, V_1, V_2] and the (n, 4) proof over
 * [V_0, V_1, V_2, identity] are the same statement.  Whoever needs the count bound binds the transaction's output list
 * outside the proof.  (Presented with outs = 3, a proof made over four real outputs is a VerificationError.)
 * Errors in addition: BPP_E_ARG naming i for outs_of[i] = 0 or above the engine's m; nothing is enqueued or written then.
 * Every *_workspace_bytes below is 0 for an outs_of that is not taken.
 *
 * bpp_outs_shapes: the rule as a function, for callers that frame streams.  Host only, no device, no context.
 * m_of_out[i] = 2^ceil(log2 outs_of[i]); BPP_E_ARG naming i for outs_of[i] = 0 or above cap_m; count = 0 is BPP_OK.
 * bpp_outputs_make* need no ragged form: they are per output, j < outs_of[i]. */
int bpp_outs_shapes(const uint32_t *outs_of, size_t count, size_t cap_m, uint32_t *m_of_out);

/* bpp_range_prove_batch_serialized_mixed[_device] over a ragged block: d_v, d_gamma hold sum(outs) entries, the commitment
 * buffer gets sum(outs) encodings, the containers are those of the shapes bpp_outs_shapes names.  flags: BPP_SER_TRANSCRIPT |
 * BPP_SER_UNCOMPRESSED | BPP_PROVE_AMOUNT64. */
size_t bpp_prover_serialized_outs_workspace_bytes(const bpp_verifier *engine, const uint32_t *outs_of, size_t count);
int bpp_range_prove_batch_serialized_outs_device(bpp_verifier *engine, const uint64_t *d_v, const uint64_t *d_gamma,
                                                 const uint32_t *outs_of, size_t count, int flags, const uint8_t *blind_key,
                                                 uint64_t index_base, const uint64_t *d_blinding, void *d_out_proofs,
                                                 void *d_out_commitments, void *d_workspace, size_t workspace_bytes,
                                                 void *stream);
int bpp_range_prove_batch_serialized_outs(bpp_verifier *engine, const uint64_t *v, const uint64_t *gamma, const uint32_t *outs_of,
                                          size_t count, int flags, const uint8_t *blind_key, uint64_t index_base,
                                          uint8_t *out_proofs, uint8_t *out_commitments);

/* bpp_range_verify_batch_serialized_mixed[_device] over a ragged block: d_ok is 0, 1 or 2 in caller order, FormatError first
 * as there.  A container whose header m is not the M of outs_of[i] is a FormatError of that proof only. */
size_t bpp_verifier_serialized_outs_workspace_bytes(const bpp_verifier *v, const uint32_t *outs_of, size_t count);
int bpp_range_verify_batch_serialized_outs_device(bpp_verifier *v, const void *d_proofs, const void *d_commitments,
                                                  const uint32_t *outs_of, size_t count, int flags, uint32_t *d_ok,
                                                  void *d_workspace, size_t workspace_bytes, void *stream);
int bpp_range_verify_batch_serialized_outs(bpp_verifier *v, const uint8_t *proofs, const uint8_t *commitments,
                                           const uint32_t *outs_of, size_t count, int flags, uint32_t *out_ok);

/* bpp_range_verify_batch_serialized_grouped_mixed_device over a ragged block: the same front, the grouped back end. */
size_t bpp_verifier_serialized_grouped_outs_workspace_bytes(const bpp_verifier *v, const uint32_t *outs_of, size_t count,
                                                            uint32_t group);
int bpp_range_verify_batch_serialized_grouped_outs_device(bpp_verifier *v, const void *d_proofs, const void *d_commitments,
                                                          const uint32_t *outs_of, size_t count, int flags,
                                                          const uint8_t *weight_key, uint64_t index_base, uint32_t group,
                                                          uint32_t *d_ok, uint64_t *stats, void *d_workspace,
                                                          size_t workspace_bytes, void *stream);

/* bpp_range_verify_find_outputs_serialized_mixed_keys[_device] over a ragged block: d_sealed and d_tags are per REAL output
 * (sum of outs_of[i] entries), output numbers in hit records count real outputs only, o = (sum of outs_of[i'] over i' < i) + j
 * with j < outs_of[i], and the pair bound is n_keys x sum(outs).  d_ok is word for word the verify call's above. */
size_t bpp_verify_find_outputs_outs_workspace_bytes(const bpp_verifier *v, const uint32_t *outs_of, size_t count, size_t n_keys);
int bpp_range_verify_find_outputs_serialized_outs_keys_device(bpp_verifier *v, const void *d_proofs, const void *d_commitments,
                                                              const uint32_t *outs_of, size_t count, int flags,
                                                              const uint8_t *d_keys, size_t n_keys, uint64_t index_base,
                                                              const uint64_t *d_index, const uint64_t *d_sealed,
                                                              const uint8_t *d_tags, uint32_t *d_ok, uint32_t *d_hits,
                                                              size_t max_hits, uint32_t *d_n_hits, uint32_t *d_n_candidates,
                                                              void *d_workspace, size_t workspace_bytes, void *stream);
int bpp_range_verify_find_outputs_serialized_outs_keys(bpp_verifier *v, const uint8_t *proofs, const uint8_t *commitments,
                                                       const uint32_t *outs_of, size_t count, int flags, const uint8_t *keys,
                                                       size_t n_keys, uint64_t index_base, const uint64_t *index,
                                                       const uint64_t *sealed, const uint8_t *tags, uint32_t *out_ok,
                                                       uint32_t *out_hits, size_t max_hits, uint32_t *out_n_hits,
                                                       uint32_t *out_n_candidates);

/* ---- the weighted inner product argument as a seam of its own: WeightedInnerProductProof::{prove, verify} ----
 * Reference: src/weighted_inner_product_proof.rs:36-227 (prove), :238-328 (verify), :330-382 (verification_scalars).
 * An engine created for (n, m) proves and verifies the WIP relation over its key for ANY statement that ends in one; only
 * len = n m counts, k = log2(len):
 *     P = sum a_i G_i + sum b_i H_i + (sum a_i b_i y^(i+1)) g + gamma h
 * power_of_y_vec is [y, y^2, .., y^len] (exp_iter_type2(y, len)): the reference's verify reads only its first entry and
 * rebuilds the rest (:252, :276) and both callers of its prove pass exactly this vector, so the seam takes the one scalar y
 * per proof.  prove's `commitment` argument is dead in the reference (:57, :137-142) and is not taken.
 *
 * The record of a proof is the one bpp_verifier_run reads: [A', wip.A, wip.B, L_0.., R_0.., V_0..V_{nv-1}], 3 + 2k + nv wire
 * points, 0 <= nv <= 64 (nv need not be a power of two).  The PROVER writes points 1 .. 2 + 2k of every record and leaves
 * point 0 and the last nv alone: the caller, who knows A' and V, fills them, and the prover's output is the verifier's input.
 *   d_a, d_b         : count x len scalars          d_y, d_gamma : count scalars (scalars >= r are reduced)
 *   d_out_scalars    : count x 3 scalars [r', s', delta']
 *   flags            : 0: the reference's literals (e_t = 7, e = 99; d_L, d_R = 4, 5; r, s, delta, eta = 33, 44, 88, 123).
 *                      BPP_SER_TRANSCRIPT: the argument continues a transcript the CALLER owns: d_transcript holds 32 bytes
 *                      per proof, the running SHA-256 state of csrc/transcript.hpp after the caller absorbed its statement
 *                      and drew y.  The engine appends dsep "wipp v1\0" and n = len (u64), per round L_t, R_t and draws e_t,
 *                      then wA, wB and draws e.  d_transcript is ignored without the flag.
 *   blinding         : d_blinding, count x (5 + 2k) scalars [unused, r, s, delta, eta, d_L[0..k), d_R[0..k)] (slot 0 is
 *                      ignored), or blind_key (32 bytes, host) expanded with index_base + i as bpp_range_prove_batch_fs_device
 *                      does, or -- both NULL -- the literals.  Blinding without BPP_SER_TRANSCRIPT, or both sources, is
 *                      BPP_E_ARG.
 *   d_out_challenges : NULL, or count x (1 + k) scalars [e, e_1..e_k] as drawn
 * y = 0 (mod r) has no inverse: the prover's output for that proof is unspecified (its neighbours are not disturbed).
 *
 * The VERIFIER takes the statement as the four *_exp_of_commitment arguments of :238-247,
 *   d_statement      : count x (2 len + 1 + nv) scalars [Gc (len), Hc (len), gc, Vc (nv)]
 * and checks the MulVec of :298-320 in the reference's order,
 *   scalars [1, e, e^2, g_exp, h_exp, e_j^2 e^2 (k), e_j^-2 e^2 (k), G_exp (len), H_exp (len), V_exp (nv)]
 *   points  [B, A, A', g, h, L.., R.., G_vec, H_vec, V..]
 *   G_exp[i] = -s[i] y^-(i+1) r' e y + Gc[i] e^2        H_exp[i] = -s[len-1-i] s' e + Hc[i] e^2
 *   g_exp = -r' y s' + gc e^2        h_exp = -delta'        V_exp[j] = Vc[j] e^2        (s[i]: :372-380)
 * d_ok[i] = 0 iff the sum is the identity (ristretto255: the engine's class test); a proof with y = 0 gets 1.
 *   d_challenges     : NULL, or count x (1 + k) scalars [e, e_1..e_k] for a caller with a transcript of its own; it takes
 *                      precedence over flags.  Otherwise BPP_SER_TRANSCRIPT derives them from d_transcript and the record.
 *                      Values >= r are taken as their residue mod r (so are d_y, d_scalars and d_statement); for an e_t
 *                      that is 0 mod r the inverse e_t^-1 is taken as 0, and the other proofs of the batch are unaffected.
 *   d_out_scalars    : NULL, or count x N scalars, N = 2 len + 2k + 5 + nv, in MulVec order; d_out_result: NULL, or the sum
 *                      per proof -- both as for bpp_verifier_run, as is bpp_verifier_set_subgroup_check.
 * Both device calls only enqueue on `stream` (no host synchronisation, no host-side upload).  Errors: BPP_E_ARG for a NULL
 * required pointer, nv > 64, a workspace that is too small, BPP_SER_TRANSCRIPT without d_transcript, the blinding rules, an
 * unknown flag; nothing is enqueued or written then.  count = 0 is BPP_OK.  The size calls return 0 for arguments that are
 * not taken.  Kernels: k_wip_init, k_wvs_prepare / k_wvs_expand, k_wip_transcript_challenges (csrc/wip_seam.hpp); everything
 * else is the range passes' own. */
size_t bpp_wip_prover_workspace_bytes(const bpp_verifier *engine, size_t count);
int bpp_wip_prove_batch_device(bpp_verifier *engine, const uint64_t *d_a, const uint64_t *d_b, const uint64_t *d_y,
                               const uint64_t *d_gamma, size_t count, size_t nv, int flags, const void *d_transcript,
                               const uint8_t *blind_key, uint64_t index_base, const uint64_t *d_blinding,
                               uint64_t *d_out_points, uint64_t *d_out_scalars, uint64_t *d_out_challenges, void *d_workspace,
                               size_t workspace_bytes, void *stream);
size_t bpp_wip_verifier_workspace_bytes(const bpp_verifier *v, size_t count, size_t nv);
int bpp_wip_verify_batch_device(bpp_verifier *v, const uint64_t *d_points, const uint64_t *d_scalars, const uint64_t *d_y,
                                const uint64_t *d_statement, size_t nv, size_t count, int flags, const void *d_transcript,
                                const uint64_t *d_challenges, uint32_t *d_ok, void *d_workspace, size_t workspace_bytes,
                                uint64_t *d_out_scalars, uint64_t *d_out_result, void *stream);
/* Both on HOST buffers, synchronous.  `points` of the prover is read AND written: count x (3 + 2k + nv) wire points whose
 * point 0 and last nv come back as they went in.  blinding, out_challenges, out_scalars (verify), out_result may be NULL. */
int bpp_wip_prove_batch(bpp_verifier *engine, const uint64_t *a, const uint64_t *b, const uint64_t *y, const uint64_t *gamma,
                        size_t count, size_t nv, int flags, const void *transcript, const uint8_t *blind_key,
                        uint64_t index_base, const uint64_t *blinding, uint64_t *points, uint64_t *out_scalars,
                        uint64_t *out_challenges);
int bpp_wip_verify_batch(bpp_verifier *v, const uint64_t *points, const uint64_t *scalars, const uint64_t *y,
                         const uint64_t *statement, size_t nv, size_t count, int flags, const void *transcript,
                         const uint64_t *challenges, uint32_t *out_ok, uint64_t *out_scalars, uint64_t *out_result);

/* Frames a bare byte stream of concatenated containers (host memory; no device, no context): m_of[i] = the m of container
 * i, whose length its header implies (n, m, k, version).  BPP_OK with *out_count containers when the stream is consumed
 * exactly (an empty stream: 0).  Otherwise a negative code, *out_count = the containers before the offending one, and
 * "container <index> at byte <offset>: <why>" in bpp_last_error(): BPP_E_LENGTH for a header that cannot be walked (bad
 * magic, a version, curve or n other than asked for, m not a power of two, k != log2(n m), a truncated tail), BPP_E_ARG
 * when there are more than max_count containers or for a curve / version / n (a power of two <= 255) that has no
 * container.  It validates only what it needs to find the next container and never reads beyond proofs_bytes; the
 * reserved bytes, the encodings and the scalars stay the decoder's business. */
int bpp_proofs_scan(int curve_id, size_t n, int version, const uint8_t *proofs, size_t proofs_bytes, uint32_t *m_of,
                    size_t max_count, size_t *out_count);

/* ---- verifier pool: ONE batch sharded over the devices of a node, behind the C ABI ----------------------------------
 * Proofs are independent units (reference src/range/mod.rs:503-509: each proof ends in its own check), so a batch is cut
 * into contiguous slices, one per shard, every shard runs the existing device pass over its slice on its own device and
 * host thread, and the verdicts come back in caller order.  The only data that cross devices are the verdict words and,
 * for the combined check, one partial of bpp_verifier_partial_bytes() bytes per shard ("a single reduce for the final
 * multiscalar check").  No kernel is added: the hot path is the passes above, run concurrently.
 *
 * THE CUT.  bpp_shard_cuts writes world + 1 cuts; shard r takes proofs [cuts[r], cuts[r + 1]): contiguous, in caller
 * order, possibly empty.  cuts[0] = 0, cuts[world] = count.
 *   m_of == NULL (uniform batch): base, rem = divmod(count, world), cuts[r] = r base + min(r, rem).
 *   otherwise proof i costs m_of[i] (n is fixed and a pass costs ~ n m_i): cuts[r], 0 < r < world, is the smallest i with
 *   world * sum_{j<i} m_of[j] >= r * sum_all m_of[j], in 64-bit arithmetic.  The cuts are monotone and every shard costs
 *   less than total / world + max m.
 * BPP_E_ARG: world = 0 or > 16, out_cuts NULL, count >= 2^32, an m_of[i] = 0 (the text names i).  Pure host code.
 *
 * THE POOL.  The handle is an opaque pointer, passed as void * like the streams of this header.  bpp_pool_create takes
 * 1 <= n_dev <= 16 ordinals and builds, concurrently, per shard r one context and one verifier of capacity (n, m) on
 * devices[r] (arguments as for bpp_init / bpp_verifier_create), with a non-blocking stream of its own.  An ordinal may
 * appear more than once: the shards then share that device -- the way to exercise a pool on a one-GPU machine.  On any
 * failure everything built is destroyed, *out stays NULL, and the code and text of the LOWEST failing shard are returned,
 * the text prefixed "shard r (device d): " (BPP_E_NOMEM for tables that do not fit, BPP_E_HIP for "no such HIP device").
 * Each shard owns its device input, verdict and workspace buffers; they grow on demand and are reused across calls.
 * bpp_pool_device: the ordinal of a shard, -1 if out of range.  bpp_pool_verifier: *out = the shard's verifier, BORROWED
 * (it dies with the pool), for callers who hold device buffers and use the _device entries, or who set
 * bpp_verifier_set_subgroup_check on each shard before a call; BPP_E_ARG and *out = NULL if out of range.
 * A pool is used by ONE host thread at a time; the borrowed verifiers follow their own rules above.  Worker threads are
 * started per call and joined before it returns.
 *
 * THE VERIFY CALLS take host pointers, are synchronous and give verdicts in caller order.
 *   bpp_pool_verify_mixed: layout and semantics of bpp_range_verify_batch_mixed (packed records, the reference's literal
 *     challenges); m_of == NULL: every proof has the capacity m.  out_ok is, word for word, what the single-verifier call
 *     writes for the whole batch.
 *   bpp_pool_verify_serialized_mixed: layout, flags and statuses 0 / 1 / 2 of bpp_range_verify_batch_serialized_mixed;
 *     m_of is required (bpp_proofs_scan recovers it from a bare stream).
 *       mode = BPP_POOL_EXACT  : each shard runs bpp_range_verify_batch_serialized_mixed_device over its slice;
 *                                weight_key, group and stats are ignored and may be NULL / 0.
 *       mode = BPP_POOL_GROUPED: each shard runs bpp_range_verify_batch_serialized_grouped_mixed_device with
 *                                index_base + cuts[r], so proof i of the caller's numbering is weighted by
 *                                PRF(weight_key, index_base + i) whatever the cut.  weight_key (32 bytes) is required,
 *                                group is a power of two >= 2.  Groups are formed INSIDE a shard, and stats = [groups
 *                                that failed, proofs re-verified exactly] is the sum over the shards: stats therefore
 *                                DEPEND ON THE CUT (on the number of shards); the statuses do not.
 *     The 4 GiB limits on container and commitment bytes apply per shard.
 *   bpp_pool_verify_combined: the combined check of a uniform batch at the capacity shape, literal challenges.  Shard r
 *     runs bpp_verifier_run_combined with index_base + cuts[r]; the partials of the non-empty shards are copied to shard
 *     0's device (a peer copy; no peer access needs enabling) and summed there by bpp_verifier_sum_partials.
 *     *out_ok (one word) = 0 iff the sum is the identity and no shard saw an invalid point; count = 0 gives 0.
 *     weight_key (32 bytes) is required.
 * Errors.  Argument errors are found before any thread starts and return BPP_E_ARG: a NULL pool or required pointer,
 * count >= 2^32, an m_of[i] that is zero, not a power of two or above the capacity (the text names the CALLER's index i),
 * an unknown flag or mode, a missing key, a bad group.  A runtime failure in a shard returns the code of the lowest
 * failing shard with the prefixed text.  In both cases out_ok and stats are not written: the shards write into the pool's
 * own host buffer, which is copied out only when every shard returned BPP_OK.  count = 0 is BPP_OK.  After a HIP
 * failure (BPP_E_HIP) the pool is usable only for bpp_pool_destroy. */
#define BPP_POOL_EXACT 0
#define BPP_POOL_GROUPED 1
int bpp_shard_cuts(const uint32_t *m_of, size_t count, size_t world, size_t *out_cuts);
int bpp_pool_create(int curve_id, const int *devices, size_t n_dev, const uint64_t *gh, const uint64_t *G, const uint64_t *H,
                    size_t n, size_t m, int window_bits, void **out);
void bpp_pool_destroy(void *pool);
size_t bpp_pool_size(const void *pool);
int bpp_pool_device(const void *pool, size_t shard);
int bpp_pool_verifier(void *pool, size_t shard, bpp_verifier **out);
int bpp_pool_verify_mixed(void *pool, const uint64_t *points, const uint64_t *scalars, const uint32_t *m_of, size_t count,
                          uint32_t *out_ok);
int bpp_pool_verify_serialized_mixed(void *pool, const uint8_t *proofs, const uint8_t *commitments, const uint32_t *m_of,
                                     size_t count, int flags, int mode, const uint8_t *weight_key, uint64_t index_base,
                                     uint32_t group, uint32_t *out_ok, uint64_t *stats);
int bpp_pool_verify_combined(void *pool, const uint64_t *points, const uint64_t *scalars, size_t count,
                             const uint8_t *weight_key, uint64_t index_base, uint32_t *out_ok);

/* name of the kernel that dominates bpp_verifier_run (for profilers) and its launch geometry */
const char *bpp_verifier_dominant_kernel(void);

#ifdef __cplusplus
}
#endif
#endif /* BPP_AMD_H */
