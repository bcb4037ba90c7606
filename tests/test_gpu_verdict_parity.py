"""-m gpu: every verify entry point of the engine against the definition verdict on one adversarial corpus
(tests/verdict_corpus.py, checked on the host by tests/test_verdict_corpus_cpu.py).

  * RangeProof.verify (bpp_range_verify): the table-free first call, the cached engine of later calls, the cache off --
    the definition verdict for every case, points outside G1 and the cancelling pair included
  * bpp_verifier_run / bpp_range_verify_batch / graph replay, subgroup check on and off; the grouped and combined checks;
    grouped begin / finish with two batches in flight; the challenges from the transcript
  * the compressed records and the serialized containers (v1, v2, transcript; host, device, grouped device)
  * the literal prove / verify lifecycle over more keys than the cache holds
  * the host scalar reduction on edwards25519: s = 2^256 - 1 on a point with an order-8 component
Each curve and shape runs in a context of its own (the verify cache belongs to the context)."""

import hashlib

import numpy as np
import pytest

import oracle as O
import pyref as P
import verdict_corpus as VC
from gpu_util import need_gpu, run_combined_device, run_grouped_device, run_verifier_device

pytestmark = pytest.mark.gpu

CURVES = ("bls12_381", "secp256k1", "ed25519")
MATRIX = [(c, s) for c in CURVES for s in VC.SHAPES]


def _engine(cp, window_bits=5):
    import bulletproofsplus_amd as B
    a = B.Arith(cp.cname)
    pk = B.PublicKey.from_points(a, cp.gh, cp.G, cp.H)
    assert np.array_equal(pk.G_vec, cp.G) and np.array_equal(pk.H_vec, cp.H)
    return B, a, pk


def _literal(B, pk, cp, c):
    try:
        B.RangeProof.from_wire(c.pts, c.sc).verify(pk, cp.n, c.V)
        return 0
    except B.VerificationError:
        return 1


def _raw_expect(cp, c, check):
    """bpp_verifier_run: the definition, except that with the subgroup check a point outside G1 is an invalid point"""
    if cp.cname == "bls12_381" and c.shifted:
        return 1 if check else None
    return c.expect


def _layout(cases, count):
    """indices into cases, `count` long: invalid cases at 0, at the last index and around the group boundaries 2, 4, 32"""
    bad = [i for i, c in enumerate(cases) if c.expect]
    idx = [(i + bad[0]) % len(cases) for i in range(count)]
    for pos in (0, 1, 2, 3, 4, 31, 32, 33, count - 1):
        if pos < count and pos % 3 != 1:
            idx[pos] = bad[pos % len(bad)]
    return idx


@pytest.mark.parametrize("cname,shape", MATRIX)
def test_literal_verify_every_path(cname, shape):
    """call 1 of a key = table-free naive MulVec, call 2 builds the tables, later calls use them; and the cache off"""
    need_gpu()
    cp = VC.corpus(cname, *shape)
    B, a, pk = _engine(cp)
    exp = [c.expect for c in cp.cases]
    first = [_literal(B, pk, cp, c) for c in cp.cases]        # case 0 on the naive path, then cached
    again = [_literal(B, pk, cp, c) for c in cp.cases]
    a.set_verify_cache(False)
    naive = [_literal(B, pk, cp, c) for c in cp.cases]
    a.set_verify_cache(True)
    names = [c.name for c in cp.cases]
    for got in (first, again, naive):
        assert got == exp, [(n, g, e) for n, g, e in zip(names, got, exp) if g != e]


@pytest.mark.parametrize("cname,shape", MATRIX)
def test_raw_verifier_matrix(cname, shape):
    torch = need_gpu()
    cp = VC.corpus(cname, *shape)
    B, a, pk = _engine(cp)
    bv = B.BatchVerifier(pk, cp.n, cp.m, window_bits=5)
    cases = [c for c in cp.cases if c.k_ok]
    recs_all = np.stack([np.concatenate([c.pts, c.V]) for c in cases])
    scs_all = np.stack([c.sc for c in cases])
    for check in (True, False):
        bv.set_subgroup_check(check)
        want = [_raw_expect(cp, c, check) for c in cases]
        for count in (len(cases), 1, 37):
            idx = list(range(len(cases))) if count == len(cases) else _layout(cases, count)
            if count == 1:
                names = [c.name for c in cases]
                idx = [names.index("R0_plus_T") if "R0_plus_T" in names else
                       next(i for i, c in enumerate(cases) if c.expect)] if check else [0]
            recs, scs = recs_all[idx], scs_all[idx]
            ok, osc, ores = run_verifier_device(torch, bv, recs, scs)
            for j, i in enumerate(idx):
                c = cases[i]
                if want[i] is not None:
                    assert ok[j] == want[i], (check, count, j, c.name, ok[j], want[i])
                if c.enc_ok and c.mv_scalars is not None:
                    assert O.wire_to_scalars(osc[j]) == c.mv_scalars, (c.name, j)
                if c.in_group and c.result is not None and (c.mv_scalars is not None):
                    assert O.wire_to_point(cp.cid, ores[j]) == c.result, (c.name, j)
            if count == len(cases):
                host = bv.verify_wire(recs, scs)         # bpp_range_verify_batch
                assert [int(x) for x, w in zip(host, want) if w is not None] == [w for w in want if w is not None]
    # graph replay of a captured pass (subgroup check on), then the grouped checks on the same layout
    bv.set_subgroup_check(True)
    want = [_raw_expect(cp, c, True) for c in cases]
    idx = _layout(cases, 37)
    recs, scs = np.ascontiguousarray(recs_all[idx]), np.ascontiguousarray(scs_all[idx])
    wv = [want[i] for i in idx]
    dev = torch.device("cuda:0")
    d_pts = torch.from_numpy(recs.view(np.int64)).to(dev)
    d_sc = torch.from_numpy(scs.view(np.int64)).to(dev)
    d_ok = torch.full((37,), 7, dtype=torch.int32, device=dev)
    wsb = bv.workspace_bytes(37)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g = bv.graph_capture(d_pts.data_ptr(), d_sc.data_ptr(), 37, d_ok.data_ptr(), d_ws.data_ptr(), wsb)
    for _ in range(2):
        d_ok.fill_(7)
        g.launch(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert d_ok.cpu().numpy().tolist() == wv
    g.close()
    # the weighted checks assume prime-order points modulo the identity class: edwards25519 torsion stays out of them
    keep = [j for j, i in enumerate(idx) if not (cname == "ed25519" and cases[i].shifted)]
    recs_g, scs_g, wv_g = recs[keep], scs[keep], [wv[j] for j in keep]
    for group in (2, 4, 32):
        got, failed, redone = run_grouped_device(torch, bv, recs_g, scs_g, group, seed=group)
        assert got.tolist() == wv_g, group
    # two grouped batches in flight on two streams
    key = hashlib.sha256(b"verdict corpus").digest()
    good = [i for i, c in enumerate(cases) if want[i] == 0 and not (cname == "ed25519" and c.shifted)]
    gi = [good[j % len(good)] for j in range(37)]
    batches = [(recs_all[gi], scs_all[gi], [0] * 37), (recs_g, scs_g, wv_g)]
    streams = [torch.cuda.Stream() for _ in batches]
    bufs = []
    for (r_, s_, _), st in zip(batches, streams):
        cnt = r_.shape[0]
        w = bv.grouped_workspace_bytes(cnt, 4)
        bufs.append((torch.from_numpy(np.ascontiguousarray(r_).view(np.int64)).to(dev),
                     torch.from_numpy(np.ascontiguousarray(s_).view(np.int64)).to(dev),
                     torch.full((cnt,), 7, dtype=torch.int32, device=dev), torch.empty(w, dtype=torch.uint8, device=dev), w, cnt))
    torch.cuda.synchronize()
    for (dp, ds, do, dw, w, cnt), st in zip(bufs, streams):
        bv.grouped_begin_device(dp.data_ptr(), ds.data_ptr(), cnt, key, 0, do.data_ptr(), dw.data_ptr(), w, group=4,
                                stream=st.cuda_stream)
    for (dp, ds, do, dw, w, cnt), st in zip(bufs, streams):
        bv.grouped_finish_device(dp.data_ptr(), ds.data_ptr(), cnt, do.data_ptr(), dw.data_ptr(), w, group=4,
                                 stream=st.cuda_stream)
    torch.cuda.synchronize()
    for (_, _, wv_b), (_, _, do, _, _, _) in zip(batches, bufs):
        assert do.cpu().numpy().tolist() == wv_b
    # the combined check: 0 iff every proof of the batch is valid
    assert run_combined_device(torch, bv, recs_all[gi], scs_all[gi], 3)[0] == 0
    for i, c in enumerate(cases):
        if want[i] and not (cname == "ed25519" and c.shifted):
            one = list(gi[:36]) + [i] if c.name != "flip_s" else [i] + list(gi[:6])
            assert run_combined_device(torch, bv, recs_all[one], scs_all[one], 5)[0] == 1, c.name
    bv.close()


@pytest.mark.parametrize("cname", ["bls12_381", "secp256k1"])
def test_transcript_challenges_matrix(cname):
    torch = need_gpu()
    cp = VC.corpus(cname, 8, 2, transcript=True)
    B, a, pk = _engine(cp)
    bv = B.BatchVerifier(pk, cp.n, cp.m, window_bits=5)
    idx = [1, 0, 2, 3, 4, 5, 0, 1, 2][:len(cp.cases) + 2]
    idx = [i % len(cp.cases) for i in idx]
    recs = np.ascontiguousarray(np.stack([np.concatenate([cp.cases[i].pts, cp.cases[i].V]) for i in idx]))
    scs = np.ascontiguousarray(np.stack([cp.cases[i].sc for i in idx]))
    dev = torch.device("cuda:0")
    d_pts = torch.from_numpy(recs.view(np.int64)).to(dev)
    d_ch = torch.zeros((len(idx), 3 + bv.k, 4), dtype=torch.int64, device=dev)
    bv.derive_challenges_device(d_pts.data_ptr(), len(idx), d_ch.data_ptr())
    torch.cuda.synchronize()
    ch = d_ch.cpu().numpy().view(np.uint64)
    want = [cp.cases[i].expect for i in idx]
    for check in (False, True):
        bv.set_subgroup_check(check)
        ok, osc, _ = run_verifier_device(torch, bv, recs, scs, want_result=False, challenges=ch)
        assert ok.tolist() == want
    # serialized with the transcript flag (canonical scalars only: r' + r is a FormatError there)
    ser = [c for c in cp.cases if not c.name.startswith("nc_")]
    blobs = [VC.encode_case(cp, c) for c in ser]
    st = bv.verify_serialized(np.stack([np.frombuffer(b, np.uint8) for b, _ in blobs]),
                              np.stack([np.frombuffer(m, np.uint8) for _, m in blobs]), transcript=True)
    assert st.tolist() == [c.expect for c in ser]
    bv.close()


@pytest.mark.parametrize("cname,shape", MATRIX)
def test_serialized_matrix(cname, shape):
    torch = need_gpu()
    cp = VC.corpus(cname, *shape)
    B, a, pk = _engine(cp)
    bv = B.BatchVerifier(pk, cp.n, cp.m, window_bits=5)
    ser = [c for c in cp.cases if c.status is not None]
    want = [c.status for c in ser]
    # compressed records: the decoder's restatement on every point (commitments included) and the scalar range
    cb = B.compressed_bytes(a)
    recs = np.stack([np.frombuffer(b"".join(P.compress_point(cp.curve, Pt) for Pt in
                                            O.wire_to_points(cp.cid, VC.canonical_inf(cp, np.concatenate([c.pts, c.V])))),
                                   np.uint8).reshape(-1, cb) for c in ser])
    assert bv.verify_compressed(recs, np.stack([c.sc for c in ser])).tolist() == want
    versions = (1, 2) if cname != "ed25519" else (1,)
    for version in versions:
        sv, wv = ser, want
        if version == 2:   # uncompressed points carry the off-curve and x + p coordinates to the decoder: FormatError
            bad = [c for c in cp.cases if not c.enc_ok and c.k_ok]
            assert bad
            for c in bad:
                assert P.decode_proof(cp.curve, cp.grp, cp.n, cp.m, VC.encode_case(cp, c, 2)[0], 2) is None, c.name
            sv, wv = ser + bad, want + [2] * len(bad)
        enc = [VC.encode_case(cp, c, version) for c in sv]
        proofs = np.stack([np.frombuffer(b, np.uint8) for b, _ in enc])
        comms = np.stack([np.frombuffer(m, np.uint8) for _, m in enc])
        assert bv.verify_serialized(proofs, comms, uncompressed=version == 2).tolist() == wv, version
        for count in (len(sv), 1, 37):
            idx = list(range(len(sv))) if count == len(sv) else \
                [next(i for i, s in enumerate(wv) if s)] if count == 1 else _layout(sv, 37)
            dev = torch.device("cuda:0")
            d_p = torch.from_numpy(np.ascontiguousarray(proofs[idx])).to(dev)
            d_c = torch.from_numpy(np.ascontiguousarray(comms[idx])).to(dev)
            d_ok = torch.full((count,), 7, dtype=torch.int32, device=dev)
            w = bv.serialized_workspace_bytes(count)
            d_ws = torch.empty(w, dtype=torch.uint8, device=dev)
            bv.verify_serialized_device(d_p.data_ptr(), d_c.data_ptr(), count, d_ok.data_ptr(), d_ws.data_ptr(), w,
                                        torch.cuda.current_stream().cuda_stream, uncompressed=version == 2)
            torch.cuda.synchronize()
            assert d_ok.cpu().numpy().tolist() == [wv[i] for i in idx], (version, count)
            for group in (4, 32):
                w = bv.serialized_grouped_workspace_bytes(count, group)
                d_ws = torch.empty(max(w, 256), dtype=torch.uint8, device=dev)
                d_ok.fill_(7)
                bv.verify_serialized_grouped_device(d_p.data_ptr(), d_c.data_ptr(), count, d_ok.data_ptr(), d_ws.data_ptr(), w,
                                                    weight_key=bytes(32), group=group,
                                                    stream=torch.cuda.current_stream().cuda_stream,
                                                    uncompressed=version == 2)
                torch.cuda.synchronize()
                assert d_ok.cpu().numpy().tolist() == [wv[i] for i in idx], (version, count, group)
    bv.close()


@pytest.mark.parametrize("cname", ["bls12_381", "secp256k1"])
def test_big_shape_subset(cname):
    """(64,16): valid, a tampered scalar and a moved L_0 on the literal call (all three paths) and the raw pass"""
    torch = need_gpu()
    cp = VC.corpus(cname, *VC.BIG)
    B, a, pk = _engine(cp)
    exp = [c.expect for c in cp.cases]
    assert exp == [0, 1, 1]
    assert [_literal(B, pk, cp, c) for c in cp.cases] == exp
    assert [_literal(B, pk, cp, c) for c in cp.cases] == exp
    a.set_verify_cache(False)
    assert [_literal(B, pk, cp, c) for c in cp.cases] == exp
    bv = B.BatchVerifier(pk, cp.n, cp.m, window_bits=8)
    idx = [1, 0, 0, 2, 0, 1]
    recs = np.stack([np.concatenate([cp.cases[i].pts, cp.cases[i].V]) for i in idx])
    ok, _, _ = run_verifier_device(torch, bv, recs, np.stack([cp.cases[i].sc for i in idx]), want_scalars=False,
                                   want_result=False)
    assert ok.tolist() == [exp[i] for i in idx]
    bv.close()


@pytest.mark.parametrize("cname,shape", [(c, s) for c in CURVES for s in ((8, 1), (8, 2))])
def test_literal_prove_verify_lifecycle(cname, shape):
    """five keys (one more than the cache holds) used in turn: entries are evicted and come back.  Every commitment equals
    the oracle's, every prove equals the oracle's bit for bit (fold path on a key's first call, the cached batched prover
    later, the fold fallback when the commitments are not those of (v, gamma)); every verify returns the definition
    verdict.  gamma = 2^256 - 1 is 15 multiples of r past r on edwards25519: the host reduction of both prover paths.
    Then again with the cache off."""
    need_gpu()
    import bulletproofsplus_amd as B
    n, m = shape
    cp = VC.corpus(cname, n, m)
    r = cp.r
    a = B.Arith(cname)
    perms = [list(range(n * m))]
    for t in range(1, 5):
        p_ = list(range(n * m))
        p_[0], p_[t] = p_[t], p_[0]
        perms.append(p_)
    keys = [B.PublicKey.from_points(a, cp.gh, cp.G[p_], cp.H) for p_ in perms]
    wits = [([0, (1 << n) - 1], [0, r - 1]), ([200, 5], [(1 << 256) - 1, 7]), ([9, 1 << 31], [3, (1 << 256) - 1]),
            ([17, 3], [r - 1, 0])]
    pool = [c for c in cp.cases if c.k_ok]

    def run_sequence():
        step = 0
        for rnd in range(3):
            for ki in (0, 1, 2, 3, 4, 2, 0):
                pk = keys[ki]
                vals, gams = (w[:m] for w in wits[(rnd + ki) % len(wits)])
                pr = B.RangeProver.new()
                for v, g in zip(vals, gams):
                    pr.commit(pk, v, g)       # gamma >= r: reduced by the engine
                for v, g, Vw in zip(vals, gams, pr.commitment_vec):
                    assert np.array_equal(Vw, cp.commit(v, g)), (rnd, ki, v, g)
                mismatch = rnd == 1 and ki == 3
                if mismatch:     # commitments that are not those of (v, gamma): the fold path reproduces the reference
                    pr.commitment_vec[m - 1] = cp.commit(6, 1)
                proof = B.RangeProof.prove(pk, n, pr)
                opts, osc, oV = cp.prove(vals, gams, perm=perms[ki], V=np.stack(pr.commitment_vec))
                assert np.array_equal(oV, np.stack(pr.commitment_vec))
                assert np.array_equal(proof.points_wire(), opts) and np.array_equal(proof.scalars_wire(), osc), \
                    (rnd, ki, mismatch)
                own = cp.verdict(opts, osc, oV, perm=perms[ki])
                assert _literal(B, pk, cp, VC.Case("own", opts, osc, oV)) == own, (rnd, ki)
                sample = pool[step % len(pool)::11][:3] + ([c for c in pool if c.shifted] if ki == 0 else [])
                for c in sample:
                    ref = c.expect if ki == 0 else (cp.verdict(c.pts, c.sc, c.V, perm=perms[ki]) if c.enc_ok else 1)
                    assert _literal(B, pk, cp, c) == ref, (rnd, ki, c.name)
                step += 1

    run_sequence()
    a.set_verify_cache(False)
    run_sequence()


def test_ed25519_host_scalar_reduction_on_torsion_point():
    """bpp_msm / bpp_msm_batch / bpp_scalar_mul_batch reduce a scalar >= r on the host; on edwards25519 2^256 - 1 holds
    15 multiples of r, and on a point with an order-8 component an incomplete reduction gives another point"""
    need_gpu()
    import bulletproofsplus_amd as B
    a = B.Arith("ed25519")
    grp = VC.FastEdwards(P.ED25519)
    r = P.ED25519["r"]
    T8 = VC.ed_torsion(8)
    Q = grp.add(grp.mul(grp.base(), 123456789), T8)
    s = (1 << 256) - 1
    want = grp.mul(Q, s % r)
    assert want != grp.mul(Q, s - 4 * r)        # the old four-round host loop's value
    Qw = O.point_to_wire(2, Q)
    mv = B.MulVec(a)
    mv.add_scalar(s)
    mv.add_point(Qw)
    assert O.wire_to_point(2, mv.calculate()) == want                                            # bpp_msm
    sc = np.stack([O.int_to_limbs(s, 4), O.int_to_limbs(5, 4)])
    pts = np.stack([Qw, O.point_to_wire(2, grp.base())])
    assert O.wire_to_point(2, B.msm_batch(a, sc[:1], pts[:1], [1])[0]) == want                    # bpp_msm_batch
    assert O.wire_to_point(2, a.scalar_mul([s, 5], pts)[0]) == want                               # bpp_scalar_mul_batch
    assert O.wire_to_point(2, B.msm_pippenger(a, sc[:1], pts[:1])) == want                        # device reduction
    both = grp.add(want, grp.mul(grp.base(), 5))
    assert O.wire_to_point(2, B.msm_pippenger(a, sc, pts)) == both
    assert O.wire_to_point(2, B.msm_batch(a, sc, pts, [2])[0]) == both
