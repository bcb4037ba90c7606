"""-m gpu: RangeProof::{prove,verify} and the batch verifier through the C ABI against the oracle and the
golden fixtures.  Bit-exact: proof points/scalars, the verifier's MulVec scalars (reference MulVec order),
the MulVec result point, and the verdict."""

import numpy as np
import pytest

import oracle as O
import pyref as P
from gpu_util import need_gpu, hexpt, run_verifier_device, run_combined_device

pytestmark = pytest.mark.gpu

CID = O.CURVE_IDS


def golden_record(curve, case):
    pts = O.points_to_wire(curve, [hexpt(h) for h in case["points"]])
    V = O.points_to_wire(curve, [hexpt(h) for h in case["V"]])
    sc = O.scalars_to_wire([int(case[k], 16) for k in ("r_prime", "s_prime", "d_prime")])
    return pts, V, sc


@pytest.mark.parametrize("idx", range(8))
def test_prove_small_matches_golden(golden, idx):
    need_gpu()
    import bulletproofsplus_amd as B
    case = golden("protocol_small.json")[idx]
    cid = CID[case["curve"]]
    a = B.Arith.init(cid)
    n, m = case["n"], case["m"]
    pk = B.PublicKey.new(a, n * m)
    pr = B.RangeProver.new()
    for v, gm in zip(case["values"], case["gammas"]):
        pr.commit(pk, v, gm)
    assert O.wire_to_points(cid, np.stack(pr.commitment_vec)) == [hexpt(h) for h in case["V"]]
    proof = B.RangeProof.prove(pk, n, pr)
    exp_pts = [hexpt(case[k]) for k in ("A", "wipA", "wipB")] + [hexpt(h) for h in case["L"]] + [hexpt(h) for h in case["R"]]
    assert O.wire_to_points(cid, proof.points_wire()) == exp_pts
    assert ["%064x" % s for s in O.wire_to_scalars(proof.scalars_wire())] == [case["r_prime"], case["s_prime"], case["d_prime"]]
    if case["verify_ok"]:
        assert proof.verify(pk, n, pr.commitment_vec) is None
    else:
        with pytest.raises(B.VerificationError):
            proof.verify(pk, n, pr.commitment_vec)


def test_prove_and_verify_reference_sizes(golden):
    """main.rs (64,2) and C1 (32,1): GPU prove == golden proof, GPU verify == Ok; then tampering."""
    need_gpu()
    import bulletproofsplus_amd as B
    a = B.Arith.init("bls12_381")
    for case in golden("protocol_full_bls12_381.json")[:2]:
        n, m = case["n"], case["m"]
        pk = B.PublicKey.new(a, n * m)
        pr = B.RangeProver.new()
        for v, gm in zip(case["values"], case["gammas"]):
            pr.commit(pk, v, gm)
        proof = B.RangeProof.prove(pk, n, pr)
        gpts, gV, gsc = golden_record(0, case)
        assert np.array_equal(proof.points_wire(), gpts)
        assert np.array_equal(proof.scalars_wire(), gsc)
        assert np.array_equal(np.stack(pr.commitment_vec), gV)
        assert proof.verify(pk, n, pr.commitment_vec) is None          # main.rs:56 assert_eq!(result, Ok(()))
        bad = B.RangeProof.from_wire(gpts, gsc)
        bad.proof.d_prime = bad.proof.d_prime.copy()
        bad.proof.d_prime[0] ^= 1
        with pytest.raises(B.VerificationError):
            bad.verify(pk, n, pr.commitment_vec)
        # the README's calling convention (README.md:47-55): RangeVerifier::new(), allocate(..), verify(.., &verifier)
        rv = B.RangeVerifier.new()
        rv.allocate(pr.commitment_vec)
        assert proof.verify(pk, n, rv) is None
        with pytest.raises(B.VerificationError):
            bad.verify(pk, n, rv)
        # wrong commitment
        V2 = np.stack(pr.commitment_vec).copy()
        V2[0] = pk.gh[0]
        with pytest.raises(B.VerificationError):
            proof.verify(pk, n, V2)
        # wrong number of rounds -> VerificationError (wip.rs:335-337)
        short = B.RangeProof.from_wire(np.concatenate([gpts[:3], gpts[3:3 + proof.proof.L_vec.shape[0] - 1],
                                                       gpts[3 + proof.proof.L_vec.shape[0]:-1]]), gsc)
        with pytest.raises(B.VerificationError):
            short.verify(pk, n, pr.commitment_vec)


@pytest.mark.parametrize("cname,n,vals,gams,c", [
    ("bls12_381", 8, [200, 5], [3, 7], 4),
    ("bls12_381", 8, [77], [9], 5),
    ("secp256k1", 8, [200, 5], [3, 7], 7),
    ("secp256k1", 8, [77], [9], 3),
    ("bls12_381", 4, [9, 3, 15, 0], [1, 2, 3, 4], 6),
    ("bls12_381", 8, [77], [9], 17),       # the bench's window width: 15 windows, unsigned top window of 118 k entries
    ("secp256k1", 8, [77], [9], 16),       # 256-bit scalars: the top window is a full 16 bits wide
])
def test_batch_verifier_small_bit_exact(cname, n, vals, gams, c):
    """Batch of valid / tampered / out-of-range proofs: scalars, result point and verdict == oracle."""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cid = CID[cname]
    m = len(vals)
    a = B.Arith.init(cid)
    opk = O.PublicKey(cid, n * m)
    pk = B.PublicKey.from_points(a, opk.gh, opk.G, opk.H)
    bv = B.BatchVerifier(pk, n, m, window_bits=c)
    recs, scs, exp_rc, exp_sc, exp_res = [], [], [], [], []

    def add(pts, sc, V):
        rc, vsc, res = O.range_verify(opk, n, m, pts, sc, V, want_scalars=True, want_result=True)
        recs.append(np.concatenate([pts, V]))
        scs.append(sc)
        exp_rc.append(rc)
        exp_sc.append(vsc)
        exp_res.append(res)

    pts, sc, V = O.range_prove(opk, n, vals, gams)
    add(pts, sc, V)                                           # valid
    t = sc.copy(); t[0, 0] ^= 1; add(pts, t, V)                # r' tampered
    t = sc.copy(); t[1, 3] ^= 1 << 40; add(pts, t, V)          # s' tampered
    t = sc.copy(); t[2, 1] ^= 5; add(pts, t, V)                # delta' tampered
    p2 = pts.copy(); p2[0] = O.point_add(cid, pts[0], opk.gh[0]); add(p2, sc, V)      # A moved
    p2 = pts.copy(); p2[3] = pts[4] if pts.shape[0] > 4 else opk.gh[1]; add(p2, sc, V)  # L_0 replaced
    V2 = V.copy(); V2[-1] = O.point_neg(cid, V[-1]); add(pts, sc, V2)                  # commitment negated
    p2 = pts.copy(); p2[1] = O.point_to_wire(cid, None); add(p2, sc, V)                # wip.A = infinity
    outside_g1 = []
    if cname == "bls12_381":
        # (0, 2) lies on y^2 = x^3 + 4 but has order 3 (outside G1): its multiples reach infinity inside the
        # proof-point tables (k_var_tables) and must be handled.  Such a point is not an element of the protocol's group:
        # the engine evaluates the proof-point MulVec with G1's endomorphism (GLV, kernels.hpp k_var_digits), which
        # equals sum s_i P_i exactly on G1 and is merely deterministic outside it -- so for these two records the verdict
        # (reject) is compared, not the full-curve sum the oracle computes.  The serialized path rejects them at decode.
        outside_g1 = [len(recs), len(recs) + 1]
        p2 = pts.copy(); p2[2] = O.point_to_wire(cid, (0, 2)); add(p2, sc, V)
        bls_p = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
        p2 = pts.copy(); p2[0] = O.point_to_wire(cid, (0, bls_p - 2)); add(p2, sc, V)      # its negative, as A
    big = [v + (1 << n) if i == 0 else v for i, v in enumerate(vals)]                  # out of range
    bpts, bsc, bV = O.range_prove(opk, n, big, gams)
    add(bpts, bsc, bV)
    pts3, sc3, V3 = O.range_prove(opk, n, [(v * 7 + 1) % (1 << n) for v in vals], [g + 11 for g in gams])
    add(pts3, sc3, V3)                                        # a second valid proof
    ok, got_sc, got_res = run_verifier_device(torch, bv, np.stack(recs), np.stack(scs))
    assert exp_rc[0] == 0 and exp_rc[-1] == 0 and exp_rc[-2] == 1 and exp_rc[1] == 1
    assert ok.tolist() == exp_rc
    for i in range(len(recs)):
        assert np.array_equal(got_sc[i], exp_sc[i]), i
        if i not in outside_g1:
            assert np.array_equal(got_res[i], exp_res[i]), i
    # host-pointer entry point gives the same verdicts
    assert bv.verify_wire(np.stack(recs), np.stack(scs)).tolist() == exp_rc
    # an off-curve point makes that proof (only) fail
    r2 = np.stack(recs[:2] + [recs[0]]).copy()
    r2[2, 0, 0] ^= 1
    ok2 = bv.verify_wire(r2, np.stack(scs[:2] + [scs[0]]))
    assert ok2.tolist() == [0, 1, 1]


@pytest.mark.parametrize("case_idx,c", [(2, 13), (2, 8), (0, 10), (1, 11)])
def test_batch_verifier_reference_sizes(golden, case_idx, c):
    """(64,16) [C2/C4], main.rs (64,2), C1 (32,1): table path == oracle scalars, identity result, verdicts."""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    case = golden("protocol_full_bls12_381.json")[case_idx]
    n, m = case["n"], case["m"]
    a = B.Arith.init("bls12_381")
    pk = B.PublicKey.new(a, n * m)
    opk = O.PublicKey(0, n * m)
    assert np.array_equal(pk.G_vec, opk.G)
    bv = B.BatchVerifier(pk, n, m, window_bits=c)
    pts, V, sc = golden_record(0, case)
    rec = np.concatenate([pts, V])
    bad_sc = sc.copy()
    bad_sc[2, 2] ^= 1
    bad_rec = rec.copy()
    bad_rec[5] = rec[6]
    recs = np.stack([rec, rec, bad_rec, rec])
    scs = np.stack([sc, bad_sc, sc, sc])
    ok, got_sc, got_res = run_verifier_device(torch, bv, recs, scs)
    assert ok.tolist() == [0, 1, 1, 0]
    _, exp_sc, _ = O.range_verify(opk, n, m, pts, sc, V, want_scalars=True, skip_msm=True)
    assert np.array_equal(got_sc[0], exp_sc) and np.array_equal(got_sc[3], exp_sc)
    k = (pts.shape[0] - 3) // 2
    assert n * m == 1 << k
    assert got_sc.shape[1] == 2 * n * m + 2 * k + m + 5
    assert bv.msm_len == exp_sc.shape[0]
    assert a.is_zero(got_res[0]) and a.is_zero(got_res[3])
    assert not a.is_zero(got_res[1]) and not a.is_zero(got_res[2])
    if n * m <= 128:   # oracle MSM of the tampered proofs is affordable at this size: result point bit-exact
        for i, (r_, s_) in ((1, (rec, bad_sc)), (2, (bad_rec, sc))):
            rc, _, res = O.range_verify(opk, n, m, r_[:pts.shape[0]], s_, r_[pts.shape[0]:], want_result=True)
            assert rc == 1 and np.array_equal(res, got_res[i])
    # per-proof challenges equal to the reference constants give the same scalars
    k = (pts.shape[0] - 3) // 2
    ch = np.zeros((4, 3 + k, 4), dtype=np.uint64)
    ch[:, 0, 0] = 7 if m == 1 else 12
    ch[:, 1, 0] = 7 if m == 1 else 23
    ch[:, 2, 0] = 99
    ch[:, 3:, 0] = 7
    ok2, sc2, _ = run_verifier_device(torch, bv, recs, scs, challenges=ch)
    assert ok2.tolist() == [0, 1, 1, 0] and np.array_equal(sc2, got_sc)


def test_window_sizes_agree(golden):
    """size-independent property: every window width gives the same MulVec result for the same proof."""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    case = golden("protocol_full_bls12_381.json")[1]   # (32,1)
    a = B.Arith.init("bls12_381")
    pk = B.PublicKey.new(a, 32)
    pts, V, sc = golden_record(0, case)
    rec = np.concatenate([pts, V])[None]
    bad = sc.copy()
    bad[0, 0] ^= 3
    results = []
    for c in (2, 3, 6, 9, 12, 14):
        bv = B.BatchVerifier(pk, 32, 1, window_bits=c)
        ok, _, res = run_verifier_device(torch, bv, np.concatenate([rec, rec]), np.stack([sc, bad]), want_scalars=False)
        assert ok.tolist() == [0, 1]
        results.append(res[1].copy())
        bv.close()
    for r in results[1:]:
        assert np.array_equal(r, results[0])


@pytest.mark.parametrize("cname,n,vals,gams,c", [
    ("bls12_381", 8, [200, 5], [3, 7], 5),
    ("secp256k1", 8, [77], [9], 6),
])
def test_combined_check_agrees_with_per_proof_verdicts(cname, n, vals, gams, c):
    """Combined batch check (engine mode, not a reference path): passes iff every per-proof verdict of the
    reference-exact path is Ok; different seeds agree; partials of two half-batches add up to the whole."""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cid = CID[cname]
    m = len(vals)
    a = B.Arith.init(cid)
    opk = O.PublicKey(cid, n * m)
    pk = B.PublicKey.from_points(a, opk.gh, opk.G, opk.H)
    bv = B.BatchVerifier(pk, n, m, window_bits=c)
    good = []
    for t in range(6):
        pts, sc, V = O.range_prove(opk, n, [(v * (t + 3) + t) % (1 << n) for v in vals], [g + 5 * t for g in gams])
        good.append((np.concatenate([pts, V]), sc))
    recs = np.stack([g[0] for g in good])
    scs = np.stack([g[1] for g in good])
    assert bv.verify_wire(recs, scs).tolist() == [0] * 6
    for seed in (1, 2, 0xDEADBEEF):
        ok, _ = run_combined_device(torch, bv, recs, scs, seed)
        assert ok == 0
    for victim in (0, 3, 5):
        bad = scs.copy()
        bad[victim, 1, 0] ^= 1
        assert bv.verify_wire(recs, bad).tolist() == [1 if i == victim else 0 for i in range(6)]
        for seed in (1, 99):
            ok, _ = run_combined_device(torch, bv, recs, bad, seed)
            assert ok == 1
    # a moved proof point and an off-curve point are caught too
    r2 = recs.copy()
    r2[2, 3] = recs[2, 4] if recs.shape[1] > 5 else opk.gh[1]
    assert run_combined_device(torch, bv, r2, scs, 7)[0] == 1
    r3 = recs.copy()
    r3[4, 0, 0] ^= 1
    assert run_combined_device(torch, bv, r3, scs, 7)[0] == 1
    # multi-rank combine: the partials of two shards of a batch holding one bad proof do not cancel, while
    # the partials of two all-valid shards are both the identity
    dev = torch.device("cuda:0")
    bad = scs.copy()
    bad[1, 0, 0] ^= 2
    parts = []
    for lo, hi, seed in ((0, 3, 11), (3, 6, 12)):
        ok, part = run_combined_device(torch, bv, recs[lo:hi], bad[lo:hi], seed)
        parts.append(part)
    d_parts = torch.from_numpy(np.concatenate(parts)).to(dev)
    d_ok = torch.full((1,), 7, dtype=torch.int32, device=dev)
    bv.sum_partials_device(d_parts.data_ptr(), 2, d_ok.data_ptr())
    torch.cuda.synchronize()
    assert int(d_ok.item()) == 1
    parts = [run_combined_device(torch, bv, recs[lo:hi], scs[lo:hi], seed)[1] for lo, hi, seed in ((0, 3, 11), (3, 6, 12))]
    d_parts = torch.from_numpy(np.concatenate(parts)).to(dev)
    bv.sum_partials_device(d_parts.data_ptr(), 2, d_ok.data_ptr())
    torch.cuda.synchronize()
    assert int(d_ok.item()) == 0


def test_combined_check_reference_size(golden):
    """(64,16): combined check over a batch built from the golden proof (valid) and a tampered copy."""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    case = golden("protocol_full_bls12_381.json")[2]
    a = B.Arith.init("bls12_381")
    pk = B.PublicKey.new(a, 1024)
    bv = B.BatchVerifier(pk, 64, 16, window_bits=9)
    pts, V, sc = golden_record(0, case)
    rec = np.concatenate([pts, V])
    recs = np.stack([rec] * 120)
    scs = np.stack([sc] * 120)
    assert run_combined_device(torch, bv, recs, scs, 5)[0] == 0
    scs[77, 2, 1] ^= 1
    assert run_combined_device(torch, bv, recs, scs, 5)[0] == 1


@pytest.mark.parametrize("cname,n,m,c", [("bls12_381", 8, 2, 5), ("secp256k1", 8, 1, 4), ("bls12_381", 4, 4, 6)])
def test_prove_batch_matches_oracle_small(cname, n, m, c):
    """Batched device prover (scalar folding + window tables) == oracle prover, bit for bit, and its
    proofs verify (and out-of-range values fail) on the batch verifier."""
    need_gpu()
    import bulletproofsplus_amd as B
    cid = CID[cname]
    a = B.Arith.init(cid)
    opk = O.PublicKey(cid, n * m)
    pk = B.PublicKey.from_points(a, opk.gh, opk.G, opk.H)
    eng = B.BatchVerifier(pk, n, m, window_bits=c)
    r = P.CURVES[cname]["r"]
    vals = [[(37 * i + 11 * j + 5) % (1 << n) for j in range(m)] for i in range(9)]
    vals[3][0] += 1 << n                       # out of range
    vals[5][m - 1] = (1 << 40) + 3             # truncated by `v as i32` in commit, bits beyond n set
    gams = [[(i * 1000003 + j * 7919 + 1) % r if i != 4 else r - 1 - j for j in range(m)] for i in range(9)]
    pts, sc, V = eng.prove_batch(vals, gams)
    exp_ok = []
    for i in range(9):
        opts, osc, oV = O.range_prove(opk, n, vals[i], gams[i])
        assert np.array_equal(pts[i], opts), i
        assert np.array_equal(sc[i], osc), i
        assert np.array_equal(V[i], oV), i
        exp_ok.append(O.range_verify(opk, n, m, opts, osc, oV))
    recs = np.concatenate([pts, V], axis=1)
    assert eng.verify_wire(recs, sc).tolist() == exp_ok
    assert exp_ok[0] == 0 and exp_ok[3] == 1


@pytest.mark.parametrize("cname,n,m,c,count", [
    ("bls12_381", 2, 2, 3, 1),        # NF = 10: fewer generators than lanes
    ("bls12_381", 4, 8, 7, 70),       # NF = 66
    ("secp256k1", 16, 2, 9, 300),     # NF = 66, 256-bit scalars
    ("bls12_381", 16, 8, 4, 33),      # NF = 258 = 2 * 128 + 2: whole generators + left-over ones, 64 windows
    ("bls12_381", 32, 8, 11, 2500),   # NF = 514, one block per proof: 4 generators per lane + 2 spread
    ("ed25519", 8, 4, 6, 40),         # extended Edwards coordinates through the same kernels
    ("ed25519", 8, 2, 5, 320),        # > 256 proofs of a small shape: the eight-lanes-per-proof Horner, 65 windows
    ("bls12_381", 8, 2, 5, 300),      # ... and with the GLV split, 33 windows
])
def test_shapes_and_batch_sizes_sweep(cname, n, m, c, count):
    """Launch geometry sweep of k_fixed_msm (lanes without generators, whole + left-over generators, one or several
    blocks per proof, fold passes): verdicts for valid / tampered proofs, and the MulVec result point of a few of
    them against the oracle."""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    a = B.Arith.init(cname)
    pk = B.PublicKey.new(a, n * m)
    eng = B.BatchVerifier(pk, n, m, window_bits=c)
    rnd = np.random.RandomState(n * 1000 + m * 10 + c)
    vals = rnd.randint(0, min(2**31 - 1, 2**n), size=(count, m)).astype(np.uint64)
    gams = [[int(x) for x in row] for row in rnd.randint(1, 2**62, size=(count, m))]
    pts, sc, V = eng.prove_batch(vals, gams)
    recs = np.concatenate([pts, V], axis=1)
    bad = sorted(set(rnd.choice(count, size=max(1, count // 7), replace=False).tolist()))
    dsc = sc.copy()
    for t, i in enumerate(bad):
        dsc[i, t % 3, rnd.randint(4)] ^= np.uint64(1) << np.uint64(rnd.randint(60))
    ok, _, res = run_verifier_device(torch, eng, recs, dsc, want_scalars=False)
    assert ok.tolist() == [1 if i in bad else 0 for i in range(count)]
    assert all(a.is_zero(res[i]) for i in range(count) if i not in bad)
    if cname != "ed25519":   # the C oracle has no Edwards backend
        cid = CID[cname]
        opk = O.PublicKey(cid, n * m)
        for i in ([0] + bad)[:3]:
            rc, _, exp = O.range_verify(opk, n, m, pts[i], dsc[i], V[i], want_result=True)
            assert rc == (1 if i in bad else 0) and np.array_equal(res[i], exp), i
    eng.close()


def test_prove_batch_reference_sizes(golden):
    """(64,2) main.rs, (32,1) and (64,16): batched prover == golden proofs; a distinct batch verifies."""
    need_gpu()
    import bulletproofsplus_amd as B
    a = B.Arith.init("bls12_381")
    for case, c in zip(golden("protocol_full_bls12_381.json"), (9, 8, 10)):
        n, m = case["n"], case["m"]
        pk = B.PublicKey.new(a, n * m)
        eng = B.BatchVerifier(pk, n, m, window_bits=c)
        gpts, gV, gsc = golden_record(0, case)
        vals = [case["values"], [(v * 3 + 1) % (1 << 31) for v in case["values"]]]
        gams = [case["gammas"], [g + 9 for g in case["gammas"]]]
        pts, sc, V = eng.prove_batch(vals, gams)
        assert np.array_equal(pts[0], gpts) and np.array_equal(sc[0], gsc) and np.array_equal(V[0], gV)
        recs = np.concatenate([pts, V], axis=1)
        assert eng.verify_wire(recs, sc).tolist() == [0, 0]
        # the single-proof API gives the same second proof
        pr = B.RangeProver.new()
        for v, g in zip(vals[1], gams[1]):
            pr.commit(pk, v, g)
        if n * m <= 128:
            proof = B.RangeProof.prove(pk, n, pr)
            assert np.array_equal(proof.points_wire(), pts[1]) and np.array_equal(proof.scalars_wire(), sc[1])
        eng.close()


def test_cpp_mirror_runs_the_reference_demo(golden):
    """include/bpp_amd.hpp (C++ host mirror of PublicKey / RangeProver / RangeProof / MulVec) running the
    reference's demo driver src/main.rs:6-56; proof scalars == golden."""
    need_gpu()
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "host", "mirror_main")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(root, "tests", "host", "mirror_main.cpp"),
                           "-L" + os.path.join(root, "bulletproofsplus_amd"), "-lbpp_amd",
                           "-Wl,-rpath," + os.path.join(root, "bulletproofsplus_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    kv = dict(line.split("=", 1) for line in out.stdout.strip().splitlines())
    case = golden("protocol_full_bls12_381.json")[0]
    assert kv["r_prime"] == case["r_prime"] and kv["s_prime"] == case["s_prime"] and kv["d_prime"] == case["d_prime"]
    assert kv["verify"] == "Ok(())" and kv["tampered"] == "Err(VerificationError)"
    assert kv["mulvec_mismatch"] == "panic" and kv["two_g_is_h"] == "1"


def test_full_size_batch_round_trip_properties():
    """BASELINE size (n=64, m=16), 256 distinct proofs: size-independent properties instead of a CPU oracle
    (the oracle needs ~0.6 s per verify at this size): prove -> verify is Ok for every proof; flipping one
    bit anywhere in a proof's scalars or swapping two of its points makes exactly that proof fail; the
    combined check accepts the clean batch and rejects the dirty one; verdicts do not depend on the window
    width of the tables."""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    a = B.Arith.init("bls12_381")
    pk = B.PublicKey.new(a, 1024)
    rnd = np.random.RandomState(5)
    count = 256
    vals = rnd.randint(0, 2**31 - 1, size=(count, 16)).astype(np.uint64)
    gams = [[int(x) for x in row] for row in rnd.randint(1, 2**62, size=(count, 16))]
    verdicts = []
    for c in (11, 14):
        eng = B.BatchVerifier(pk, 64, 16, window_bits=c)
        if c == 11:
            pts, sc, V = eng.prove_batch(vals, gams)
            recs = np.concatenate([pts, V], axis=1)
            dirty_sc = sc.copy()
            dirty_recs = recs.copy()
            bad = sorted(rnd.choice(count, size=40, replace=False).tolist())
            for t, i in enumerate(bad):
                if t % 2 == 0:
                    dirty_sc[i, t % 3, rnd.randint(4)] ^= np.uint64(1) << np.uint64(rnd.randint(60))
                else:
                    j = 3 + (t % 10)
                    dirty_recs[i, [j, j + 10]] = dirty_recs[i, [j + 10, j]]      # L_j <-> R_j
        assert eng.verify_wire(recs, sc).tolist() == [0] * count
        v = eng.verify_wire(dirty_recs, dirty_sc).tolist()
        assert v == [1 if i in bad else 0 for i in range(count)]
        verdicts.append(v)
        assert run_combined_device(torch, eng, recs, sc, 3 + c)[0] == 0
        assert run_combined_device(torch, eng, dirty_recs, dirty_sc, 3 + c)[0] == 1
        if c == 14:
            # 768 proofs: three blocks per proof (stride 384), so 130 of the 2 050 generators are left over and
            # are spread over the lanes in 6 extra steps of k_fixed_msm; 256 proofs above: 8 blocks, 1 extra step
            v3 = eng.verify_wire(np.tile(dirty_recs, (3, 1, 1)), np.tile(dirty_sc, (3, 1, 1))).tolist()
            assert v3 == v * 3
        eng.close()
    assert verdicts[0] == verdicts[1]


@pytest.mark.parametrize("cname,n,vals,gams", [("bls12_381", 8, [200, 5], [3, 7]), ("secp256k1", 8, [77], [9]),
                                               ("ed25519", 4, [9, 3, 15, 0], [1, 2, 3, 4])])
def test_arbitrary_per_proof_challenges(cname, n, vals, gams, monkeypatch):
    """The verifier is not tied to the reference's constant "transcript": with full-width per-proof
    challenges (y, z, e, one e_t per round) supplied through d_challenges, the MulVec scalars, result and
    verdict equal the big-integer restatement run with the same challenges.  (The reference itself has no
    transcript; this is the path a Fiat-Shamir front end would use.)"""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cid = CID[cname]
    m = len(vals)
    mn = n * m
    k = mn.bit_length() - 1
    r = P.CURVES[cname]["r"]
    a = B.Arith.init(cid)
    G = P.make_group(cname, shadow=False)
    recs, scs, chs, exp_sc, exp_ok = [], [], [], [], []
    for t in range(3):
        y = (0x1234567890ABCDEF1234567890ABCDEF * (t + 3) ** 7 + 11) % r
        z = (0xFEDCBA0987654321FEDCBA0987654321 * (t + 5) ** 5 + 7) % r
        ef = (0xA5A5A5A5DEADBEEFCAFEBABE12345678 * (t + 2) ** 9 + 3) % r
        er = [(0x9E3779B97F4A7C15F39CC0605CEDC834 * (i + 2 + t) ** 11 + 1) % r for i in range(k)]
        for name, val in (("Y_SINGLE", y), ("Z_SINGLE", z), ("Y_MULTI", y), ("Z_MULTI", z), ("E_FINAL", ef), ("E_ROUND", er)):
            monkeypatch.setattr(P.Transcript, name, val)
        pk = P.PublicKey(G, mn)
        pr = P.RangeProver()
        for v, g in zip(vals, gams):
            pr.commit(pk, v, g + t)
        proof = P.RangeProof.prove(pk, n, pr)
        mv = proof.verify_mulvec(pk, n, pr.commitment_vec)
        exp_ok.append(0 if proof.verify(pk, n, pr.commitment_vec) else 1)
        exp_sc.append(mv.scalars)
        pts = [proof.A, proof.proof.A, proof.proof.B] + proof.proof.L_vec + proof.proof.R_vec + pr.commitment_vec
        recs.append(O.points_to_wire(cid, pts))
        scs.append(O.scalars_to_wire([proof.proof.r_prime, proof.proof.s_prime, proof.proof.d_prime]))
        chs.append(O.scalars_to_wire([y, z, ef] + er))
    assert exp_ok == [0, 0, 0]
    ppk = P.PublicKey(G, mn)
    pk = B.PublicKey.from_points(a, O.points_to_wire(cid, [ppk.g, ppk.h]), O.points_to_wire(cid, ppk.G_vec),
                                 O.points_to_wire(cid, ppk.H_vec))
    bv = B.BatchVerifier(pk, n, m, window_bits=5)
    ok, got_sc, got_res = run_verifier_device(torch, bv, np.stack(recs), np.stack(scs), challenges=np.stack(chs))
    assert ok.tolist() == [0, 0, 0]
    for t in range(3):
        assert O.wire_to_scalars(got_sc[t]) == exp_sc[t], t
    # the same proofs under the reference's constants (or each other's challenges) do not verify
    ok2, _, _ = run_verifier_device(torch, bv, np.stack(recs), np.stack(scs))
    assert ok2.tolist() == [1, 1, 1]
    ok3, _, _ = run_verifier_device(torch, bv, np.stack(recs), np.stack(scs), challenges=np.stack(chs[::-1]))
    assert ok3.tolist() == [1, 0, 1]


def test_secp256k1_reference_size_against_oracle():
    """secp256k1 at n = 64, m = 4 (mn = 256): batched prover == C oracle prover, verifier scalars == oracle."""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    a = B.Arith.init("secp256k1")
    opk = O.PublicKey(O.SECP256K1, 256)
    pk = B.PublicKey.new(a, 256)
    assert np.array_equal(pk.G_vec, opk.G)
    vals, gams = [31, 2**31 - 1, 0, 123456789], [7, 8, 9, 10]
    opts, osc, oV = O.range_prove(opk, 64, vals, gams)
    eng = B.BatchVerifier(pk, 64, 4, window_bits=9)
    pts, sc, V = eng.prove_batch([vals], [gams])
    assert np.array_equal(pts[0], opts) and np.array_equal(sc[0], osc) and np.array_equal(V[0], oV)
    rc, exp_sc, _ = O.range_verify(opk, 64, 4, opts, osc, oV, want_scalars=True, skip_msm=True)
    rec = np.concatenate([opts, oV])[None]
    ok, got_sc, got_res = run_verifier_device(torch, eng, rec, osc[None])
    assert ok.tolist() == [0] and np.array_equal(got_sc[0], exp_sc) and a.is_zero(got_res[0])


def test_maximum_supported_shape_round_trip():
    """n = 64, m = 64 (mn = 4096, k = 12, 8 285 MulVec terms, 91 proof points): the largest shape the engine
    accepts.  Exercises the > 64 KB dynamic-LDS path of k_vs_expand and NV > 64 in the proof-point
    kernels.  Round trip + tamper + combined check; shapes beyond the limit are usage errors."""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    a = B.Arith.init("bls12_381")
    pk = B.PublicKey.new(a, 4096)
    eng = B.BatchVerifier(pk, 64, 64, window_bits=8)
    assert eng.msm_len == 2 * 4096 + 24 + 64 + 5 and eng.points_per_proof == 91
    rnd = np.random.RandomState(9)
    vals = rnd.randint(0, 2**31 - 1, size=(3, 64)).astype(np.uint64)
    gams = [[int(x) for x in row] for row in rnd.randint(1, 2**62, size=(3, 64))]
    pts, sc, V = eng.prove_batch(vals, gams)
    recs = np.concatenate([pts, V], axis=1)
    assert eng.verify_wire(recs, sc).tolist() == [0, 0, 0]
    bad = sc.copy()
    bad[1, 0, 2] ^= 1
    assert eng.verify_wire(recs, bad).tolist() == [0, 1, 0]
    assert run_combined_device(torch, eng, recs, sc, 1)[0] == 0
    assert run_combined_device(torch, eng, recs, bad, 1)[0] == 1
    # shadow known answer for the first proof's scalars (group independent)
    _, _, sproof = P.prove_case("bls12_381", 64, [int(x) for x in vals[0]], gams[0], shadow=True)
    assert O.wire_to_scalars(sc[0]) == [sproof.proof.r_prime, sproof.proof.s_prime, sproof.proof.d_prime]
    with pytest.raises(B.BppError):
        B.BatchVerifier(B.PublicKey.new(a, 24), 8, 3, window_bits=8)       # n*m not a power of two
    with pytest.raises(B.BppError):
        B.BatchVerifier(pk, 64, 64, window_bits=40)                         # window out of range
