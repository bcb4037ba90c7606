"""-m gpu: one engine of capacity (n, m) PROVES a block in which proof i has m_i values (bpp_range_prove_batch_mixed_device,
bpp_range_prove_batch_serialized_mixed_device and their host forms).

Proof i must be, bit for bit, RangeProof::prove for PublicKey::new(n m_i), the prefix key of its own shape: checked against
the C oracle (BLS12-381, secp256k1; literal mode, and under the transcript with blinding from a key at the CALLER's index),
against dedicated (n, m_i) engines on all three curves, as bytes against pyref's container encoder of the oracle's proof
(edwards25519: pyref's own prover), on the (64, 16) capacity with a class that spans several prover chunks and the golden
proof inside the block, and for the usage errors.  The outputs are fed UNCHANGED to the mixed verify entries."""

import hashlib

import numpy as np
import pytest

import oracle as O
import verdict_corpus as VC
from gpu_util import need_gpu, hexpt

pytestmark = pytest.mark.gpu

CURVES = ("bls12_381", "secp256k1", "ed25519")
N, CAP, WB = 8, 4, 5
CLASSES = (1, 2, 4)
# every class next to every other one, in both orders; blocks start and end with different classes
MS = [1, 2, 4, 1, 4, 2, 2, 1, 4, 4, 2, 1, 1, 4, 2]


def _k(m, n=N):
    return (n * m).bit_length() - 1


def _nv(m, n=N):
    return 3 + 2 * _k(m, n) + m


def _gathered(ms):
    """gathered position of every caller position: classes in ascending m, caller order inside a class"""
    order = sorted(range(len(ms)), key=lambda i: (ms[i], i))
    pos = [0] * len(ms)
    for g, i in enumerate(order):
        pos[i] = g
    return pos


def _witness(ms, r, n=N):
    """values / gammas per proof; in every class the second proof holds an out-of-range value and the third one a value
    above 2^31 (the `v as i32` quirk of the commitment)"""
    vals, gams, seen = [], [], {}
    for i, m in enumerate(ms):
        t = seen[m] = seen.get(m, 0) + 1
        v = [(37 * i + 11 * j + 5) % (1 << n) for j in range(m)]
        if t == 2:
            v[0] += 1 << n
        if t == 3:
            v[m - 1] = (1 << 40) + 3
        vals.append(v)
        gams.append([(i * 1000003 + j * 7919 + 1) % r if t != 4 else r - 1 - j for j in range(m)])
    return vals, gams


def _setup(cname, n=N, cap=CAP, wb=WB):
    import bulletproofsplus_amd as B
    cps = {m: VC.Corpus(cname, n, m, False) for m in CLASSES if m <= cap}
    a = B.Arith(cname)
    bv = B.BatchVerifier(B.PublicKey.from_points(a, cps[cap].gh, cps[cap].G, cps[cap].H), n, cap, window_bits=wb)
    return B, a, bv, cps


def _dedicated(B, a, cps, m, n=N, wb=WB):
    cap = cps[max(cps)]
    return B.BatchVerifier(B.PublicKey.from_points(a, cap.gh, cap.G[:n * m], cap.H[:n * m]), n, m, window_bits=wb)


def _dev(torch, x):
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.uint8).reshape(-1)).to(torch.device("cuda:0"))


def _pack(B, vals, gams):
    v = np.array([int(x) for row in vals for x in row], dtype=np.uint64)
    g = O.scalars_to_wire([int(x) for row in gams for x in row])
    return v, g


def _prove_wire(torch, B, bv, vals, gams, transcript=False, blind_key=None, index_base=0, blinding=None, fill=0x5a):
    """the device entry -> (packed points (sum NV_i, PW), scalars (count, 3, 4), packed challenges (sum 3 + k_i, 4))"""
    ms = [len(v) for v in vals]
    PW = bv.arith.PW
    v, g = _pack(B, vals, gams)
    d_v, d_g = _dev(torch, v), _dev(torch, g)
    npts, nch = sum(_nv(m, bv.n) for m in ms), sum(3 + _k(m, bv.n) for m in ms)
    d_p = torch.full((npts * PW * 8,), fill, dtype=torch.uint8, device="cuda:0")
    d_s = torch.full((len(ms) * 96,), fill, dtype=torch.uint8, device="cuda:0")
    d_c = torch.full((nch * 32,), fill, dtype=torch.uint8, device="cuda:0")
    d_b = _dev(torch, blinding) if blinding is not None else None
    wsb = bv.prover_mixed_workspace_bytes(ms)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    bv.prove_mixed_device(d_v.data_ptr(), d_g.data_ptr(), ms, d_p.data_ptr(), d_s.data_ptr(), d_ws.data_ptr(), wsb,
                          torch.cuda.current_stream().cuda_stream, transcript=transcript, d_out_challenges=d_c.data_ptr(),
                          blind_key=blind_key, index_base=index_base, d_blinding=d_b.data_ptr() if d_b is not None else 0)
    torch.cuda.synchronize()
    return (d_p.cpu().numpy().view(np.uint64).reshape(npts, PW), d_s.cpu().numpy().view(np.uint64).reshape(len(ms), 3, 4),
            d_c.cpu().numpy().view(np.uint64).reshape(nch, 4), d_p, d_s, d_c)


def _split(pts, ms, n=N):
    off = np.concatenate([[0], np.cumsum([_nv(m, n) for m in ms])]).astype(int)
    return [pts[off[i]:off[i + 1]] for i in range(len(ms))]


def _verify_wire(torch, bv, d_p, d_s, ms, d_ch=None):
    wsb = bv.mixed_workspace_bytes(ms)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    d_ok = torch.full((len(ms),), 7, dtype=torch.int32, device="cuda:0")
    bv.run_mixed_device(d_p.data_ptr(), d_s.data_ptr(), ms, d_ok.data_ptr(), d_ws.data_ptr(), wsb,
                        torch.cuda.current_stream().cuda_stream, d_challenges=d_ch.data_ptr() if d_ch is not None else 0)
    torch.cuda.synchronize()
    return d_ok.cpu().tolist()


def _prove_bytes(torch, B, bv, vals, gams, transcript=False, uncompressed=False, blind_key=None, index_base=0, fill=0x5a):
    """the device entry -> (proof bytes, commitment bytes, device buffers)"""
    ms = [len(v) for v in vals]
    v, g = _pack(B, vals, gams)
    d_v, d_g = _dev(torch, v), _dev(torch, g)
    version = 2 if uncompressed else 1
    pb = B.uncompressed_bytes(bv.arith) if uncompressed else B.compressed_bytes(bv.arith)
    nbytes = sum(B.proof_bytes(bv.arith, bv.n, m, version) for m in ms)
    d_p = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda:0")
    d_c = torch.full((sum(ms) * pb,), fill, dtype=torch.uint8, device="cuda:0")
    wsb = bv.prover_mixed_workspace_bytes(ms, serialized=True)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    bv.prove_serialized_mixed_device(d_v.data_ptr(), d_g.data_ptr(), ms, d_p.data_ptr(), d_c.data_ptr(), d_ws.data_ptr(), wsb,
                                     torch.cuda.current_stream().cuda_stream, transcript=transcript, uncompressed=uncompressed,
                                     blind_key=blind_key, index_base=index_base)
    torch.cuda.synchronize()
    return d_p.cpu().numpy().tobytes(), d_c.cpu().numpy().tobytes(), d_p, d_c


def _verify_bytes(torch, bv, d_p, d_c, ms, transcript=False, uncompressed=False):
    wsb = bv.serialized_mixed_workspace_bytes(ms)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    d_ok = torch.full((len(ms),), 7, dtype=torch.int32, device="cuda:0")
    bv.verify_serialized_mixed_device(d_p.data_ptr(), d_c.data_ptr(), ms, d_ok.data_ptr(), d_ws.data_ptr(), wsb,
                                      torch.cuda.current_stream().cuda_stream, transcript=transcript, uncompressed=uncompressed)
    torch.cuda.synchronize()
    return d_ok.cpu().tolist()


def test_block_is_interleaved():
    """a condition of the tests below: every class next to every other one, and most proofs gathered elsewhere"""
    pairs = {(a, b) for a, b in zip(MS, MS[1:]) if a != b}
    assert pairs == {(a, b) for a in CLASSES for b in CLASSES if a != b}
    moved = sum(1 for i, g in enumerate(_gathered(MS)) if i != g)
    assert moved > len(MS) // 2, moved
    assert all(MS.count(m) >= 4 for m in CLASSES)


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_mixed_block_matches_oracle(cname):
    """literal mode: every record, scalar triple and commitment equals the oracle's proof under the prefix key of the proof's
    own shape; the output buffers, unchanged, through the mixed verifier give the oracle's verdicts"""
    torch = need_gpu()
    B, a, bv, cps = _setup(cname)
    vals, gams = _witness(MS, cps[CAP].r)
    pts, sc, ch, d_p, d_s, d_c = _prove_wire(torch, B, bv, vals, gams)
    want_ok = []
    for i, (m, rec) in enumerate(zip(MS, _split(pts, MS))):
        opts, osc, oV = O.range_prove(cps[m].opk, N, vals[i], gams[i])
        assert np.array_equal(rec[:3 + 2 * _k(m)], opts), (i, m)
        assert np.array_equal(rec[3 + 2 * _k(m):], oV), (i, m)
        assert np.array_equal(sc[i], osc), (i, m)
        want_ok.append(int(O.range_verify(cps[m].opk, N, m, opts, osc, oV)))
    assert 0 in want_ok and 1 in want_ok
    for m in CLASSES:   # an out-of-range proof in every class
        assert {want_ok[i] for i in range(len(MS)) if MS[i] == m} == {0, 1}, m
    assert _verify_wire(torch, bv, d_p, d_s, MS) == want_ok
    # literal challenges, written out on request: the verifier given them agrees with the verifier that defaults to them
    assert _verify_wire(torch, bv, d_p, d_s, MS, d_c) == want_ok
    bv.close()


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_transcript_and_key_follow_the_caller_index(cname):
    torch = need_gpu()
    B, a, bv, cps = _setup(cname)
    r = cps[CAP].r
    vals, gams = _witness(MS, r)
    key = hashlib.sha256(b"prove mixed blinding key").digest()
    base = (1 << 33) + 17
    pts, sc, ch, d_p, d_s, d_c = _prove_wire(torch, B, bv, vals, gams, transcript=True, blind_key=key, index_base=base)
    recs = _split(pts, MS)
    want_ok, blinds = [], []
    O.set_transcript(True)
    try:
        for i, m in enumerate(MS):
            bl = O.blinding_from_key(key, base + i, _k(m), r)
            blinds.append(bl)
            O.set_blinding(bl)
            opts, osc, oV = O.range_prove(cps[m].opk, N, vals[i], gams[i])
            assert np.array_equal(recs[i][:3 + 2 * _k(m)], opts), (i, m)
            assert np.array_equal(recs[i][3 + 2 * _k(m):], oV) and np.array_equal(sc[i], osc), (i, m)
            want_ok.append(int(O.range_verify(cps[m].opk, N, m, opts, osc, oV)))
    finally:
        O.set_blinding(None)
        O.set_transcript(False)
    assert 0 in want_ok and 1 in want_ok
    # d_out_challenges is what the verifier derives from the output
    wsb = bv.mixed_workspace_bytes(MS)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    d_ch2 = torch.zeros_like(d_c)
    bv.derive_challenges_mixed_device(d_p.data_ptr(), MS, d_ch2.data_ptr(), d_ws.data_ptr(), wsb,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(d_c, d_ch2)
    assert _verify_wire(torch, bv, d_p, d_s, MS, d_c) == want_ok
    # the same expansions handed in as d_blinding (packed 5 + 2 k_i per proof): identical proofs
    packed = O.scalars_to_wire([x for bl in blinds for x in bl])
    pts2, sc2, ch2 = _prove_wire(torch, B, bv, vals, gams, transcript=True, blinding=packed)[:3]
    assert np.array_equal(pts2, pts) and np.array_equal(sc2, sc) and np.array_equal(ch2, ch)
    # the same values at two caller indices: different proofs, equal commitments
    twice = [vals[2], vals[1], vals[2]]
    gtw = [gams[2], gams[1], gams[2]]
    p3, s3 = _prove_wire(torch, B, bv, twice, gtw, transcript=True, blind_key=key, index_base=base)[:2]
    r3 = _split(p3, [len(v) for v in twice])
    kk = 3 + 2 * _k(len(twice[0]))
    assert np.array_equal(r3[0][kk:], r3[2][kk:])
    assert not np.array_equal(r3[0][:kk], r3[2][:kk]) and not np.array_equal(s3[0], s3[2])
    # ... and proofs 1 and 2 sit at the caller indices they had in the block above: the same proofs
    assert np.array_equal(r3[1], recs[1]) and np.array_equal(r3[2], recs[2]) and not np.array_equal(r3[0], recs[2])
    bv.close()


@pytest.mark.parametrize("cname", CURVES)
def test_mixed_block_equals_dedicated_engines(cname):
    torch = need_gpu()
    B, a, bv, cps = _setup(cname)
    vals, gams = _witness(MS, cps[CAP].r)
    for transcript in (False, True):
        pts, sc = _prove_wire(torch, B, bv, vals, gams, transcript=transcript)[:2]
        recs = _split(pts, MS)
        for m in CLASSES:
            pos = [i for i in range(len(MS)) if MS[i] == m]
            ded = _dedicated(B, a, cps, m)
            dp, ds, dV = ded.prove_batch([vals[i] for i in pos], [gams[i] for i in pos], transcript=transcript)
            for j, i in enumerate(pos):
                assert np.array_equal(recs[i], np.concatenate([dp[j], dV[j]])), (transcript, m, i)
                assert np.array_equal(sc[i], ds[j]), (transcript, m, i)
            ded.close()
            # a block of one class; for the capacity class it is the engine's own prove_batch
            p1, s1 = _prove_wire(torch, B, bv, [vals[i] for i in pos], [gams[i] for i in pos], transcript=transcript)[:2]
            assert np.array_equal(p1, np.concatenate([recs[i] for i in pos])) and np.array_equal(s1, sc[pos])
            if m == CAP:
                cp_, cs_, cV_ = bv.prove_batch([vals[i] for i in pos], [gams[i] for i in pos], transcript=transcript)
                assert np.array_equal(p1.reshape(len(pos), -1, a.PW), np.concatenate([cp_, cV_], axis=1))
                assert np.array_equal(s1, cs_)
                if cname != "ed25519" and not transcript:   # the existing prove_batch still equals the oracle
                    for j, i in enumerate(pos):
                        opts, osc, oV = O.range_prove(cps[m].opk, N, vals[i], gams[i])
                        assert np.array_equal(cp_[j], opts) and np.array_equal(cs_[j], osc) and np.array_equal(cV_[j], oV)
    bv.close()


@pytest.mark.parametrize("cname,version", [(c, 1) for c in CURVES] + [("bls12_381", 2), ("secp256k1", 2)])
def test_bytes_match_the_reference_encoding(cname, version):
    torch = need_gpu()
    B, a, bv, cps = _setup(cname)
    vals, gams = _witness(MS, cps[CAP].r)
    unc = version == 2
    raw, cm, d_p, d_c = _prove_bytes(torch, B, bv, vals, gams, uncompressed=unc)
    blobs, comms, want_ok = [], [], []
    for i, m in enumerate(MS):
        opts, osc, oV = cps[m].prove(vals[i], gams[i])          # the oracle; edwards25519: pyref's prover
        blob, comm = VC.encode_case(cps[m], VC.Case("p", opts, osc, oV), version)
        assert len(blob) == B.proof_bytes(a, N, m, version)
        blobs.append(blob)
        comms.append(comm)
        want_ok.append(cps[m].verdict(opts, osc, oV))
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(int)
    coff = np.concatenate([[0], np.cumsum([len(c) for c in comms])]).astype(int)
    for i in range(len(MS)):
        assert raw[off[i]:off[i + 1]] == blobs[i], (i, MS[i])
        assert cm[coff[i]:coff[i + 1]] == comms[i], (i, MS[i])
    assert raw == b"".join(blobs) and cm == b"".join(comms)
    assert B.proofs_scan(a, N, raw, version).tolist() == MS
    assert 0 in want_ok and 1 in want_ok
    ok = _verify_bytes(torch, bv, d_p, d_c, MS, uncompressed=unc)
    assert ok == want_ok and 2 not in ok
    # one flipped byte in one container afterwards: that proof's status only
    for j in (0, 6, len(MS) - 1):
        at = int(off[j + 1]) - 40          # inside s'
        d_p[at] ^= 1
        bad = _verify_bytes(torch, bv, d_p, d_c, MS, uncompressed=unc)
        d_p[at] ^= 1
        assert bad[j] != ok[j] or ok[j] == 1, j
        assert [x for t, x in enumerate(bad) if t != j] == [x for t, x in enumerate(ok) if t != j], j
    # the first in-range proof: flipped, it no longer verifies
    j = want_ok.index(0)
    d_p[int(off[j + 1]) - 40] ^= 1
    assert _verify_bytes(torch, bv, d_p, d_c, MS, uncompressed=unc)[j] != 0
    bv.close()


def test_bytes_under_the_transcript_and_version_2_on_ristretto():
    torch = need_gpu()
    B, a, bv, cps = _setup("bls12_381")
    vals, gams = _witness(MS, cps[CAP].r)
    key = hashlib.sha256(b"k").digest()
    raw, cm, d_p, d_c = _prove_bytes(torch, B, bv, vals, gams, transcript=True, blind_key=key, index_base=9)
    w = _prove_wire(torch, B, bv, vals, gams, transcript=True, blind_key=key, index_base=9)
    pts, sc = w[:2]
    recs = _split(pts, MS)
    want = b"".join(B.encode_proofs(a, N, m, recs[i][None, :3 + 2 * _k(m)], sc[i][None]).tobytes() for i, m in enumerate(MS))
    assert raw == want
    assert cm == b"".join(B.compress_points(a, recs[i][3 + 2 * _k(m):]).tobytes() for i, m in enumerate(MS))
    ok = _verify_bytes(torch, bv, d_p, d_c, MS, transcript=True)
    assert set(ok) == {0, 1} and ok == _verify_wire(torch, bv, w[3], w[4], MS, w[5])
    assert _verify_bytes(torch, bv, d_p, d_c, MS) != ok          # the transcript binds the proofs
    bv.close()
    B2, a2, bv2, cps2 = _setup("ed25519")
    with pytest.raises(B.BppError) as ei:
        _prove_bytes(torch, B2, bv2, vals, gams, uncompressed=True)
    assert ei.value.code == -1
    with pytest.raises(B.BppError):
        bv2.prove_serialized_mixed(vals, gams, uncompressed=True)
    bv2.close()


def test_capacity_64_16(golden):
    """capacity (64, 16), window 8, BLS12-381: 4 096 x m = 1 (more than one prover chunk), 256 x m = 16 and 64 each of
    m = 2, 4, 8, permuted; byte-identical to the dedicated (64, 1) engine's and the capacity engine's prove_batch; the golden
    (64, 16) proof inside the block; everything verifies through run_mixed_device"""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    n, M = 64, 16
    case = golden("protocol_full_bls12_381.json")[2]
    assert (case["n"], case["m"]) == (n, M)
    a = B.Arith("bls12_381")
    pk = B.PublicKey.new(a, n * M)
    bv = B.BatchVerifier(pk, n, M, window_bits=8)
    e1 = B.BatchVerifier(B.PublicKey.from_points(a, pk.gh, pk.G_vec[:n], pk.H_vec[:n]), n, 1, window_bits=8)
    rng = np.random.default_rng(11)
    counts = {1: 4096, 2: 64, 4: 64, 8: 64, 16: 256}
    ms = np.concatenate([np.full(c, m) for m, c in counts.items()])
    ms = ms[rng.permutation(len(ms))].tolist()
    g_at = ms.index(16, len(ms) // 2)
    vals = [rng.integers(0, 1 << 31, size=m, dtype=np.uint64).tolist() for m in ms]
    gams = [[int(x) for x in rng.integers(1, 1 << 62, size=m)] for m in ms]
    vals[g_at], gams[g_at] = list(case["values"]), list(case["gammas"])
    pos = _gathered(ms)
    assert sum(1 for i, g in enumerate(pos) if i != g) > len(ms) // 2
    assert counts[1] > 2048   # a prover chunk holds at most 2 048 proofs (prove_chunk)
    pts, sc, ch, d_p, d_s, d_c = _prove_wire(torch, B, bv, vals, gams)
    recs = _split(pts, ms, n)
    i1 = [i for i, m in enumerate(ms) if m == 1]
    p1, s1, V1 = e1.prove_batch([vals[i] for i in i1], [gams[i] for i in i1])
    assert np.array_equal(np.stack([recs[i] for i in i1]), np.concatenate([p1, V1], axis=1))
    assert np.array_equal(sc[i1], s1)
    i16 = [i for i, m in enumerate(ms) if m == 16]
    p16, s16, V16 = bv.prove_batch([vals[i] for i in i16], [gams[i] for i in i16])
    assert np.array_equal(np.stack([recs[i] for i in i16]), np.concatenate([p16, V16], axis=1))
    assert np.array_equal(sc[i16], s16)
    gpts = O.points_to_wire(0, [hexpt(h) for h in case["points"]])
    gV = O.points_to_wire(0, [hexpt(h) for h in case["V"]])
    gsc = O.scalars_to_wire([int(case[k], 16) for k in ("r_prime", "s_prime", "d_prime")])
    assert np.array_equal(recs[g_at], np.concatenate([gpts, gV])) and np.array_equal(sc[g_at], gsc)
    assert _verify_wire(torch, bv, d_p, d_s, ms) == [0] * len(ms)
    e1.close()
    bv.close()


def test_arguments():
    torch = need_gpu()
    from bulletproofsplus_amd import _lib
    B, a, bv, cps = _setup("secp256k1")
    vals, gams = _witness(MS[:6], cps[CAP].r)
    ms = MS[:6]
    v, g = _pack(B, vals, gams)
    d_v, d_g = _dev(torch, v), _dev(torch, g)
    npts = sum(_nv(m) for m in ms)
    d_p = torch.full((npts * a.PW * 8,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_s = torch.full((len(ms) * 96,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_b = torch.full((1 << 16,), 0x5a, dtype=torch.uint8, device="cuda:0")     # proofs / commitments of the byte form
    wsb = max(bv.prover_mixed_workspace_bytes(ms), bv.prover_mixed_workspace_bytes(ms, serialized=True))
    assert 0 < bv.prover_mixed_workspace_bytes(ms) < bv.prover_mixed_workspace_bytes(ms, serialized=True)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == 0x5a).all()) for t in (d_p, d_s, d_b))

    for bad_ms, where in (([1, 3, 4, 1, 4, 2], 1), ([1, 2, 4, 1, 2 * CAP, 2], 4), ([0, 2, 4, 1, 4, 2], 0)):
        assert bv.prover_mixed_workspace_bytes(bad_ms) == 0
        assert bv.prover_mixed_workspace_bytes(bad_ms, serialized=True) == 0
        with pytest.raises(B.BppError) as ei:
            bv.prove_mixed_device(d_v.data_ptr(), d_g.data_ptr(), bad_ms, d_p.data_ptr(), d_s.data_ptr(), d_ws.data_ptr(), wsb, st)
        assert ei.value.code == -1 and ("m_of[%d]" % where) in str(ei.value), str(ei.value)
        with pytest.raises(B.BppError) as ei:
            bv.prove_serialized_mixed_device(d_v.data_ptr(), d_g.data_ptr(), bad_ms, d_b.data_ptr(), d_b.data_ptr() + (1 << 15),
                                             d_ws.data_ptr(), wsb, st)
        assert ei.value.code == -1 and ("m_of[%d]" % where) in str(ei.value), str(ei.value)
        if 0 not in bad_ms:     # the wrapper takes m_i from the length of each value list
            bad_vals = [[1] * m for m in bad_ms]
            with pytest.raises(B.BppError) as ei:
                bv.prove_batch_mixed(bad_vals, bad_vals)
            assert ("m_of[%d]" % where) in str(ei.value)
            with pytest.raises(B.BppError) as ei:
                bv.prove_serialized_mixed(bad_vals, bad_vals)
            assert ("m_of[%d]" % where) in str(ei.value)
    with pytest.raises(B.BppError) as ei:
        bv.prove_mixed_device(d_v.data_ptr(), d_g.data_ptr(), ms, d_p.data_ptr(), d_s.data_ptr(), d_ws.data_ptr(),
                              bv.prover_mixed_workspace_bytes(ms) - 1, st)
    assert ei.value.code == -1 and "workspace" in str(ei.value)
    with pytest.raises(B.BppError) as ei:
        bv.prove_serialized_mixed_device(d_v.data_ptr(), d_g.data_ptr(), ms, d_b.data_ptr(), d_b.data_ptr() + (1 << 15),
                                         d_ws.data_ptr(), bv.prover_mixed_workspace_bytes(ms, serialized=True) - 1, st)
    assert ei.value.code == -1 and "workspace" in str(ei.value)
    with pytest.raises(B.BppError) as ei:     # blind_key and d_blinding both given
        bv.prove_mixed_device(d_v.data_ptr(), d_g.data_ptr(), ms, d_p.data_ptr(), d_s.data_ptr(), d_ws.data_ptr(), wsb, st,
                              transcript=True, blind_key=bytes(32), d_blinding=d_b.data_ptr())
    assert ei.value.code == -1 and "both" in str(ei.value)
    m6 = bv._ms(ms)
    L = _lib.lib()
    for null_at in (1, 2, 3, 9, 10, 12):
        argv = [bv.handle, d_v.data_ptr(), d_g.data_ptr(), m6.ctypes.data, 6, 0, None, 0, None, d_p.data_ptr(), d_s.data_ptr(),
                None, d_ws.data_ptr(), wsb, None]
        argv[null_at] = None
        assert L.bpp_range_prove_batch_mixed_device(*argv) == -1, null_at
    for null_at in (1, 2, 3, 9, 10, 11):
        argv = [bv.handle, d_v.data_ptr(), d_g.data_ptr(), m6.ctypes.data, 6, 0, None, 0, None, d_b.data_ptr(),
                d_b.data_ptr() + (1 << 15), d_ws.data_ptr(), wsb, None]
        argv[null_at] = None
        assert L.bpp_range_prove_batch_serialized_mixed_device(*argv) == -1, null_at
    assert L.bpp_range_prove_batch_mixed_device(bv.handle, d_v.data_ptr(), d_g.data_ptr(), m6.ctypes.data, 6, 2, None, 0, None,
                                                d_p.data_ptr(), d_s.data_ptr(), None, d_ws.data_ptr(), wsb, None) == -1
    assert L.bpp_range_prove_batch_serialized_mixed_device(bv.handle, d_v.data_ptr(), d_g.data_ptr(), m6.ctypes.data, 6, 4, None,
                                                           0, None, d_b.data_ptr(), d_b.data_ptr() + (1 << 15), d_ws.data_ptr(),
                                                           wsb, None) == -1
    assert untouched()
    # count = 0
    bv.prove_mixed_device(d_v.data_ptr(), d_g.data_ptr(), [], d_p.data_ptr(), d_s.data_ptr(), d_ws.data_ptr(), wsb, st)
    bv.prove_serialized_mixed_device(d_v.data_ptr(), d_g.data_ptr(), [], d_b.data_ptr(), d_b.data_ptr(), d_ws.data_ptr(), wsb, st)
    assert L.bpp_range_prove_batch_mixed(bv.handle, None, None, None, 0, 0, None, 0, None, None, None) == 0
    assert L.bpp_range_prove_batch_serialized_mixed(bv.handle, None, None, None, 0, 0, None, 0, None, None) == 0
    assert bv.prove_batch_mixed([], [])[0] == [] and bv.prove_serialized_mixed([], [])[:2] == (b"", b"")
    assert untouched()
    bv.close()


@pytest.mark.parametrize("cname", ("bls12_381", "ed25519"))
def test_host_entries_and_wrappers_agree_with_the_device_entries(cname):
    torch = need_gpu()
    B, a, bv, cps = _setup(cname)
    vals, gams = _witness(MS, cps[CAP].r)
    key = hashlib.sha256(b"host").digest()
    for transcript, bk in ((False, None), (True, None), (True, key)):
        pts, sc, ch = _prove_wire(torch, B, bv, vals, gams, transcript=transcript, blind_key=bk, index_base=3)[:3]
        recs, hsc, hch = bv.prove_batch_mixed(vals, gams, transcript=transcript, blind_key=bk, index_base=3, challenges=True)
        assert [r.shape[0] for r in recs] == [_nv(m) for m in MS]
        assert np.array_equal(np.concatenate(recs), pts) and np.array_equal(hsc, sc) and np.array_equal(np.concatenate(hch), ch)
        if not transcript:
            assert bv.verify_wire_mixed(recs, hsc, MS).tolist() == _verify_wire(torch, bv, _dev(torch, pts), _dev(torch, sc), MS)
        raw, cm = _prove_bytes(torch, B, bv, vals, gams, transcript=transcript, blind_key=bk, index_base=3)[:2]
        hraw, hcm, hms = bv.prove_serialized_mixed(vals, gams, transcript=transcript, blind_key=bk, index_base=3)
        assert hraw == raw and hcm == cm and hms.tolist() == MS
        ok = bv.verify_serialized_mixed(hraw, hcm, transcript=transcript)     # framed by proofs_scan
        assert set(ok.tolist()) == {0, 1}
    bv.close()


@pytest.mark.parametrize("cname", CURVES)
def test_host_twins_at_one_proof_and_the_block_against_the_oracle(cname):
    """bpp_range_prove_batch_mixed / _serialized_mixed and the two mixed verify twins on host pointers, at one proof (m = 1,
    m = 4) and at the block of mixed m_i.  Optional inputs absent: literal mode, no key, no challenges out -- the oracle's
    proofs (pyref's on edwards25519) and their encoding byte for byte, the definition's verdicts.  Present (the Weierstrass
    curves, where the C oracle proves under a transcript): the transcript, a blinding key at the caller's index, the
    challenges out."""
    need_gpu()
    B, a, bv, cps = _setup(cname)
    r = cps[CAP].r
    vals, gams = _witness(MS, r)
    ref = [cps[m].prove(vals[i], gams[i]) for i, m in enumerate(MS)]
    enc = [VC.encode_case(cps[m], VC.Case("p", *ref[i]), 1) for i, m in enumerate(MS)]
    want_ok = [cps[m].verdict(*ref[i]) for i, m in enumerate(MS)]
    assert 0 in want_ok and 1 in want_ok
    sels = ([0], [2], list(range(len(MS))))
    assert MS[0] == 1 and MS[2] == 4
    for sel in sels:
        v_, g_, ms_ = [vals[i] for i in sel], [gams[i] for i in sel], [MS[i] for i in sel]
        blob, comm = b"".join(enc[i][0] for i in sel), b"".join(enc[i][1] for i in sel)
        hraw, hcm, hms = bv.prove_serialized_mixed(v_, g_)
        assert bytes(hraw) == blob and bytes(hcm) == comm and hms.tolist() == ms_, sel
        recs, hsc = bv.prove_batch_mixed(v_, g_)
        for j, i in enumerate(sel):
            assert np.array_equal(recs[j], np.concatenate([ref[i][0], ref[i][2]])) and np.array_equal(hsc[j], ref[i][1]), (sel, i)
        exp = [want_ok[i] for i in sel]
        assert bv.verify_wire_mixed([np.concatenate([ref[i][0], ref[i][2]]) for i in sel], np.stack([ref[i][1] for i in sel]),
                                    ms_).tolist() == exp, sel
        assert bv.verify_serialized_mixed(blob, comm, ms_).tolist() == exp, sel
    if cname != "ed25519":
        key = hashlib.sha256(b"host twins").digest()
        base = (1 << 33) + 17
        O.set_transcript(True)
        try:
            for sel in sels:
                v_, g_, ms_ = [vals[i] for i in sel], [gams[i] for i in sel], [MS[i] for i in sel]
                recs, hsc, hch = bv.prove_batch_mixed(v_, g_, transcript=True, blind_key=key, index_base=base + sel[0], challenges=True)
                hraw, hcm, _ = bv.prove_serialized_mixed(v_, g_, transcript=True, blind_key=key, index_base=base + sel[0])
                exp, blobs, comms = [], [], []
                for j, i in enumerate(sel):
                    m = MS[i]
                    O.set_blinding(O.blinding_from_key(key, base + sel[0] + j, _k(m), r))
                    opts, osc, oV = O.range_prove(cps[m].opk, N, vals[i], gams[i])
                    assert np.array_equal(recs[j], np.concatenate([opts, oV])) and np.array_equal(hsc[j], osc), (sel, i)
                    assert hch[j].shape == (3 + _k(m), 4)
                    exp.append(int(O.range_verify(cps[m].opk, N, m, opts, osc, oV)))
                    blob, comm = VC.encode_case(cps[m], VC.Case("p", opts, osc, oV), 1)
                    blobs.append(blob)
                    comms.append(comm)
                assert bytes(hraw) == b"".join(blobs) and bytes(hcm) == b"".join(comms), sel
                assert bv.verify_serialized_mixed(hraw, hcm, ms_, transcript=True).tolist() == exp, sel
        finally:
            O.set_blinding(None)
            O.set_transcript(False)
    bv.close()
