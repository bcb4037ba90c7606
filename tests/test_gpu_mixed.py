"""-m gpu: mixed batches (bpp_verifier_run_mixed) -- proof i of shape (n, m_i) against one (n, m) verifier's tables.

Each verdict must be RangeProof::verify(proof_i, PublicKey::new(n m_i), n, V_i): the definition with the PREFIX key of
the proof's own shape.  Checked against the adversarial corpus (tests/verdict_corpus.py) of every class, against
dedicated (n, m_i) verifiers bit for bit, under the transcript, on the (64, 16) headline shape with a large device-proved
batch, and for the usage errors."""

import functools

import numpy as np
import pytest

import oracle as O
import verdict_corpus as VC
from gpu_util import need_gpu, run_verifier_device

pytestmark = pytest.mark.gpu

CURVES = ("bls12_381", "secp256k1", "ed25519")
N, CAP, WB = 8, 4, 5
CLASSES = (1, 2, 4)


@functools.lru_cache(maxsize=None)
def _corpora(cname):
    return {m: VC.corpus(cname, N, m) for m in CLASSES}


def _raw_expect(cp, c, check):
    """bpp_verifier_run's verdict: the definition, except that with the subgroup check a point outside G1 is invalid"""
    if cp.cname == "bls12_381" and c.shifted:
        return 1 if check else None
    return c.expect


def _interleave(cases_by_m, order):
    """(m, case index) pairs using every case of every class: the classes alternate in the pattern a b c a c b, so that
    each sits next to each other one; the batch starts with order[0] and ends with order[-1]"""
    a, b, c = order
    pattern = [a, b, c, a, c, b]
    used = {m: 0 for m in order}
    seq = []
    while any(used[m] < len(cases_by_m[m]) for m in order) or len(seq) < 6:
        m = pattern[len(seq) % 6]
        seq.append((m, used[m] % len(cases_by_m[m])))
        used[m] += 1
    seq.append((c, 0))
    return seq


def _run_mixed(torch, bv, recs, scs, ms, challenges=None, want_result=True):
    """recs: list of per-proof (NV_i, PW) records -> (ok, result points) numpy, caller order"""
    dev = torch.device("cuda:0")
    count = len(ms)
    PW = bv.arith.PW
    pts = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.uint64).reshape(-1, PW) for r in recs]))
    d_pts = torch.from_numpy(pts.view(np.int64)).to(dev)
    d_sc = torch.from_numpy(np.ascontiguousarray(scs, dtype=np.uint64).view(np.int64)).to(dev)
    d_ok = torch.full((count,), 7, dtype=torch.int32, device=dev)
    d_or = torch.zeros((count, PW), dtype=torch.int64, device=dev) if want_result else None
    d_ch = None
    if challenges is not None:
        flat = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint64).reshape(-1) for c in challenges]))
        d_ch = torch.from_numpy(flat.view(np.int64)).to(dev)
    wsb = bv.mixed_workspace_bytes(ms)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    bv.run_mixed_device(d_pts.data_ptr(), d_sc.data_ptr(), ms, d_ok.data_ptr(), d_ws.data_ptr(), wsb,
                        torch.cuda.current_stream().cuda_stream, d_challenges=d_ch.data_ptr() if d_ch is not None else 0,
                        d_out_result=d_or.data_ptr() if d_or is not None else 0)
    torch.cuda.synchronize()
    return d_ok.cpu().numpy().astype(np.uint32), (d_or.cpu().numpy().view(np.uint64) if d_or is not None else None)


def _setup(cname):
    import bulletproofsplus_amd as B
    cps = _corpora(cname)
    cap = cps[CAP]
    a = B.Arith(cname)
    pk = B.PublicKey.from_points(a, cap.gh, cap.G, cap.H)
    bv = B.BatchVerifier(pk, N, CAP, window_bits=WB)
    cases = {m: [c for c in cps[m].cases if c.k_ok] for m in CLASSES}
    return B, a, bv, cps, cases


def _record(c):
    return np.concatenate([c.pts, c.V])


@pytest.mark.parametrize("cname", CURVES)
def test_mixed_matches_the_definition(cname):
    torch = need_gpu()
    B, a, bv, cps, cases = _setup(cname)
    cap = cps[CAP]
    # the prefix property the feature rests on: the key of (8, m') is the head of the capacity key, hashed keys too
    for m in CLASSES:
        cp = cps[m]
        assert np.array_equal(cp.gh, cap.gh)
        assert np.array_equal(cp.G, cap.G[:N * m]) and np.array_equal(cp.H, cap.H[:N * m]), m
        hk = B.PublicKey.hashed(a, N * m, b"mixed")
        hcap = B.PublicKey.hashed(a, N * CAP, b"mixed")
        assert np.array_equal(hk.gh, hcap.gh)
        assert np.array_equal(hk.G_vec, hcap.G_vec[:N * m]) and np.array_equal(hk.H_vec, hcap.H_vec[:N * m]), m
    for order in ((1, 2, 4), (2, 4, 1), (4, 1, 2)):
        seq = _interleave(cases, order)
        recs = [_record(cases[m][i]) for m, i in seq]
        scs = np.stack([cases[m][i].sc for m, i in seq])
        ms = [m for m, _ in seq]
        for check in (True, False):
            bv.set_subgroup_check(check)
            ok, res = _run_mixed(torch, bv, recs, scs, ms)
            for j, (m, i) in enumerate(seq):
                c = cases[m][i]
                want = _raw_expect(cps[m], c, check)
                if want is not None:
                    assert ok[j] == want, (order, check, j, m, c.name, ok[j], want)
                if c.in_group and c.result is not None and c.mv_scalars is not None:
                    assert O.wire_to_point(cps[m].cid, res[j]) == c.result, (order, j, m, c.name)
    bv.set_subgroup_check(False)


@pytest.mark.parametrize("cname", CURVES)
def test_mixed_equals_dedicated_verifiers(cname):
    torch = need_gpu()
    B, a, bv, cps, cases = _setup(cname)
    seq = _interleave(cases, (2, 1, 4))
    recs = [_record(cases[m][i]) for m, i in seq]
    scs = np.stack([cases[m][i].sc for m, i in seq])
    ms = [m for m, _ in seq]
    for check in (True, False):
        bv.set_subgroup_check(check)
        ok, res = _run_mixed(torch, bv, recs, scs, ms)
        for m in CLASSES:
            cp = cps[m]
            pos = [j for j, (mm, _) in enumerate(seq) if mm == m]
            ded = B.BatchVerifier(B.PublicKey.from_points(a, cp.gh, cp.G, cp.H), N, m, window_bits=WB)
            ded.set_subgroup_check(check)
            dok, _, dres = run_verifier_device(torch, ded, np.stack([recs[j] for j in pos]), scs[pos], want_scalars=False)
            assert ok[pos].tolist() == dok.tolist(), (check, m)
            assert np.array_equal(res[pos], dres), (check, m)
            ded.close()
        # a batch of one class only is that class's bpp_verifier_run
        for m in CLASSES:
            only = [cases[m][i % len(cases[m])] for i in range(5)]
            ok1, res1 = _run_mixed(torch, bv, [_record(c) for c in only], np.stack([c.sc for c in only]), [m] * 5)
            if m == CAP:
                dok, _, dres = run_verifier_device(torch, bv, np.stack([_record(c) for c in only]),
                                                   np.stack([c.sc for c in only]), want_scalars=False)
                assert ok1.tolist() == dok.tolist() and np.array_equal(res1, dres)
            assert ok1.tolist() == [_raw_expect(cps[m], c, check) if _raw_expect(cps[m], c, check) is not None
                                    else int(ok1[j]) for j, c in enumerate(only)]
    bv.set_subgroup_check(False)


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_mixed_transcript(cname):
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cps = {m: VC.corpus(cname, N, m, transcript=True) for m in CLASSES}
    cap = cps[CAP]
    a = B.Arith(cname)
    bv = B.BatchVerifier(B.PublicKey.from_points(a, cap.gh, cap.G, cap.H), N, CAP, window_bits=WB)
    cases = {m: cps[m].cases for m in CLASSES}
    seq = _interleave(cases, (4, 1, 2))
    recs = [_record(cases[m][i]) for m, i in seq]
    scs = np.stack([cases[m][i].sc for m, i in seq])
    ms = [m for m, _ in seq]
    dev = torch.device("cuda:0")
    PW = a.PW
    pts = np.ascontiguousarray(np.concatenate([r.reshape(-1, PW) for r in recs]))
    d_pts = torch.from_numpy(pts.view(np.int64)).to(dev)
    nch = [3 + (N * m).bit_length() - 1 for m in ms]
    d_ch = torch.zeros(sum(nch) * 4, dtype=torch.int64, device=dev)
    wsb = bv.mixed_workspace_bytes(ms)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    bv.derive_challenges_mixed_device(d_pts.data_ptr(), ms, d_ch.data_ptr(), d_ws.data_ptr(), wsb,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flat = d_ch.cpu().numpy().view(np.uint64)
    got, off = [], 0
    for k in nch:
        got.append(flat[off * 4:(off + k) * 4].reshape(k, 4))
        off += k
    # the oracle's challenges under the prefix key of each proof's shape, and each dedicated verifier's
    O.set_transcript(True)
    try:
        for j, (m, i) in enumerate(seq):
            c, cp = cases[m][i], cps[m]
            ch = O.range_verify(cp.opk, N, m, c.pts, c.sc_red, c.V, want_challenges=True)[-1]
            assert np.array_equal(got[j], ch), (m, c.name)
    finally:
        O.set_transcript(False)
    for m in CLASSES:
        cp = cps[m]
        pos = [j for j, (mm, _) in enumerate(seq) if mm == m]
        ded = B.BatchVerifier(B.PublicKey.from_points(a, cp.gh, cp.G, cp.H), N, m, window_bits=WB)
        sub = np.ascontiguousarray(np.stack([recs[j] for j in pos]))
        d_sub = torch.from_numpy(sub.view(np.int64)).to(dev)
        k = 3 + (N * m).bit_length() - 1
        d_dch = torch.zeros(len(pos) * k * 4, dtype=torch.int64, device=dev)
        ded.derive_challenges_device(d_sub.data_ptr(), len(pos), d_dch.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        dch = d_dch.cpu().numpy().view(np.uint64).reshape(len(pos), k, 4)
        for t, j in enumerate(pos):
            assert np.array_equal(got[j], dch[t]), (m, j)
        ded.close()
    # with those challenges, the verdicts are the definition's (the transcript corpus's own)
    ok, _ = _run_mixed(torch, bv, recs, scs, ms, challenges=got, want_result=False)
    assert ok.tolist() == [cases[m][i].expect for m, i in seq]


def test_mixed_big_shape():
    """capacity (64, 16) at window 8 on BLS12-381: the corpus's (64,16) cases beside oracle-made (64,1) and (64,2)
    proofs; then 4 096 device-proved (64,1) proofs and 256 (64,16) ones, a few tampered, against dedicated verifiers"""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cname, n, M = "bls12_381", 64, 16
    big = VC.corpus(cname, n, M)
    a = B.Arith(cname)
    pk = B.PublicKey.from_points(a, big.gh, big.G, big.H)
    bv = B.BatchVerifier(pk, n, M, window_bits=8)
    recs, scs, ms, want = [], [], [], []
    for m in (1, 2):
        opk = O.PublicKey(big.cid, n * m)
        assert np.array_equal(opk.G, big.G[:n * m]) and np.array_equal(opk.H, big.H[:n * m])
        for t in range(3):
            pts, sc, V = O.range_prove(opk, n, [(77 * t + 5 * j) % (1 << n) for j in range(m)], [3 + t + j for j in range(m)])
            sc = np.array(sc, copy=True)
            if t == 1:
                sc[1, 0] ^= 1
            recs.append(np.concatenate([pts, V]))
            scs.append(sc)
            ms.append(m)
            want.append(int(O.range_verify(opk, n, m, pts, sc, V)))
    for c in big.cases:
        recs.insert(len(recs) // 2, _record(c))
        scs.insert(len(scs) // 2, c.sc)
        ms.insert(len(ms) // 2, M)
        want.insert(len(want) // 2, c.expect)
    assert 0 in want and 1 in want
    ok, _ = _run_mixed(torch, bv, recs, np.stack(scs), ms, want_result=False)
    assert ok.tolist() == want
    # (values below 2^31: RangeProver::commit takes v as i32)
    # the large-batch geometry (Horner form 0, several blocks per proof) for the (64,1) class next to a lone (64,16) one
    rng = np.random.default_rng(7)
    pk1 = B.PublicKey.from_points(a, big.gh, big.G[:n], big.H[:n])
    e1 = B.BatchVerifier(pk1, n, 1, window_bits=8)
    p1, s1, V1 = e1.prove_batch(rng.integers(0, 1 << 31, size=(4096, 1), dtype=np.uint64).tolist(),
                                [[int(x)] for x in rng.integers(1, 1 << 62, size=4096)])
    p16, s16, V16 = bv.prove_batch(rng.integers(0, 1 << 31, size=(256, M), dtype=np.uint64).tolist(),
                                   [[int(x) for x in row] for row in rng.integers(1, 1 << 62, size=(256, M))])
    for t in (3, 1000, 4095):
        s1[t, 1, 0] ^= 1
    for t in (0, 200):
        s16[t, 1, 0] ^= 1
    r1 = np.concatenate([p1, V1], axis=1)
    r16 = np.concatenate([p16, V16], axis=1)
    order = rng.permutation(4096 + 256)
    recs = [r1[i] if i < 4096 else r16[i - 4096] for i in order]
    scs = np.stack([s1[i] if i < 4096 else s16[i - 4096] for i in order])
    ms = [1 if i < 4096 else M for i in order]
    ok, res = _run_mixed(torch, bv, recs, scs, ms)
    d1, _, dr1 = run_verifier_device(torch, e1, r1, s1, want_scalars=False)
    d16, _, dr16 = run_verifier_device(torch, bv, r16, s16, want_scalars=False)
    assert sorted(np.flatnonzero(d1).tolist()) == [3, 1000, 4095] and sorted(np.flatnonzero(d16).tolist()) == [0, 200]
    exp_ok = np.array([d1[i] if i < 4096 else d16[i - 4096] for i in order])
    exp_res = np.stack([dr1[i] if i < 4096 else dr16[i - 4096] for i in order])
    assert np.array_equal(ok, exp_ok)
    assert np.array_equal(res, exp_res)
    e1.close()
    bv.close()


def test_mixed_arguments():
    torch = need_gpu()
    from bulletproofsplus_amd import _lib
    B, a, bv, cps, cases = _setup("secp256k1")
    good = [cases[m][0] for m in CLASSES]
    recs = [_record(c) for c in good]
    scs = np.stack([c.sc for c in good])
    dev = torch.device("cuda:0")
    PW = a.PW
    pts = np.ascontiguousarray(np.concatenate([r.reshape(-1, PW) for r in recs]))
    d_pts = torch.from_numpy(pts.view(np.int64)).to(dev)
    d_sc = torch.from_numpy(np.ascontiguousarray(scs).view(np.int64)).to(dev)
    d_ok = torch.full((3,), 7, dtype=torch.int32, device=dev)
    wsb = bv.mixed_workspace_bytes(list(CLASSES))
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    for bad_ms, where in (([1, 3, 4], 1), ([1, 2, 2 * CAP], 2), ([0, 2, 4], 0)):
        assert bv.mixed_workspace_bytes(bad_ms) == 0
        with pytest.raises(B.BppError) as ei:
            bv.run_mixed_device(d_pts.data_ptr(), d_sc.data_ptr(), bad_ms, d_ok.data_ptr(), d_ws.data_ptr(), wsb, st)
        assert ei.value.code == -1 and ("m_of[%d]" % where) in str(ei.value), str(ei.value)
        with pytest.raises(B.BppError):
            bv.verify_wire_mixed(pts, scs, bad_ms)
    with pytest.raises(B.BppError) as ei:
        bv.run_mixed_device(d_pts.data_ptr(), d_sc.data_ptr(), list(CLASSES), d_ok.data_ptr(), d_ws.data_ptr(), wsb - 1, st)
    assert ei.value.code == -1 and "workspace" in str(ei.value)
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [7, 7, 7]
    bv.run_mixed_device(d_pts.data_ptr(), d_sc.data_ptr(), [], d_ok.data_ptr(), d_ws.data_ptr(), wsb, st)
    assert _lib.lib().bpp_range_verify_batch_mixed(bv.handle, None, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [7, 7, 7]
    bv.run_mixed_device(d_pts.data_ptr(), d_sc.data_ptr(), list(CLASSES), d_ok.data_ptr(), d_ws.data_ptr(), wsb, st)
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [c.expect for c in good] == [0, 0, 0]


@pytest.mark.parametrize("cname", ("bls12_381", "ed25519"))
def test_mixed_host_entry_and_wrapper(cname):
    torch = need_gpu()
    B, a, bv, cps, cases = _setup(cname)
    seq = _interleave(cases, (1, 4, 2))
    recs = [_record(cases[m][i]) for m, i in seq]
    scs = np.stack([cases[m][i].sc for m, i in seq])
    ms = [m for m, _ in seq]
    ok, _ = _run_mixed(torch, bv, recs, scs, ms, want_result=False)
    assert bv.verify_wire_mixed(recs, scs, ms).tolist() == ok.tolist()
    packed = np.concatenate([r.reshape(-1, a.PW) for r in recs])
    assert bv.verify_wire_mixed(packed, scs, ms).tolist() == ok.tolist()
    with pytest.raises(RuntimeError):
        bv.verify_wire_mixed(recs, scs, ms[:-1] + [ms[-1] * 2 if ms[-1] < CAP else 1])
    with pytest.raises(RuntimeError):
        bv.verify_wire_mixed(packed[:-1], scs, ms)
    want = [_raw_expect(cps[m], cases[m][i], False) for m, i in seq]
    assert [int(x) for x, w in zip(ok, want) if w is not None] == [w for w in want if w is not None]
