"""-m gpu: full 64-bit amounts (BPP_PROVE_AMOUNT64) on the mixed prove calls and in the literal single call, and the
batched commitment kernel (bpp_commit_batch_device / bpp_commit_batch).

The reference forms a commitment as new(v as i32) g + gamma h (src/range/prover.rs:37) while the witness bits come from the
whole u64, so its proof of an amount of 2^31 or more does not verify.  With the flag the scalar on g is the u64.  The
references here are the C oracle proving against caller-made untruncated commitments (BLS12-381, secp256k1) and pyref with
a hand-filled RangeProver (edwards25519); commitments are checked against the oracle's point arithmetic.  The library's own
other paths are compared with as well where the issue is that two of its paths agree, never as the reference."""

import functools
import hashlib
import random

import numpy as np
import pytest

import oracle as O
import verdict_corpus as VC
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

AMOUNT64 = 0x100
CID = {"bls12_381": 0, "secp256k1": 1, "ed25519": 2}
N64, WB = 64, 5
BIG = (1 << 63) + 12345
MS = [1, 2, 1]
VALS = [[BIG], [1 << 31, (1 << 64) - 1], [5]]
KEY = hashlib.sha256(b"amount64 blinding key").digest()
BASE = (1 << 33) + 5


def _k(m, n):
    return (n * m).bit_length() - 1


def _nv(m, n):
    return 3 + 2 * _k(m, n) + m


def _gammas(r):
    return [[r - 3], [(r - 1) // 2, 77], [123456789]]


def _i32(v):
    return ((v & 0xffffffff) ^ 0x80000000) - 0x80000000


@functools.lru_cache(maxsize=None)
def _corpus(cname, n, m):
    return VC.Corpus(cname, n, m, False)


def _mul_add(cp, gh, s, gamma):
    """s g + gamma h by the checker's own point arithmetic -> wire point"""
    if cp.cname != "ed25519":
        return O.point_add(cp.cid, O.point_mul(cp.cid, gh[0], s % cp.r), O.point_mul(cp.cid, gh[1], gamma % cp.r))
    g, h = O.wire_to_points(2, gh)
    return O.point_to_wire(2, cp.grp.add(cp.grp.mul(g, s % cp.r), cp.grp.mul(h, gamma % cp.r)))


def _full_commitments(cp, vals, gams):
    return np.stack([_mul_add(cp, cp.gh, v, g) for v, g in zip(vals, gams)])


def _engine(cname, n, cap, wb=WB):
    import bulletproofsplus_amd as B
    cp = _corpus(cname, n, cap)
    a = B.Arith(cname)
    bv = B.BatchVerifier(B.PublicKey.from_points(a, cp.gh, cp.G, cp.H), n, cap, window_bits=wb)
    return B, a, bv


def _dev(torch, x):
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.uint8).reshape(-1)).to(torch.device("cuda:0"))


def _pack(vals, gams):
    v = np.array([int(x) for row in vals for x in row], dtype=np.uint64)
    return v, O.scalars_to_wire([int(x) for row in gams for x in row])


def _prove_wire(torch, bv, vals, gams, amount64, transcript=False, blind_key=None, index_base=0):
    ms = [len(v) for v in vals]
    PW, n = bv.arith.PW, bv.n
    v, g = _pack(vals, gams)
    d_v, d_g = _dev(torch, v), _dev(torch, g)
    npts, nch = sum(_nv(m, n) for m in ms), sum(3 + _k(m, n) for m in ms)
    d_p = torch.full((npts * PW * 8,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_s = torch.full((len(ms) * 96,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_c = torch.full((nch * 32,), 0x5a, dtype=torch.uint8, device="cuda:0")
    wsb = bv.prover_mixed_workspace_bytes(ms)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    bv.prove_mixed_device(d_v.data_ptr(), d_g.data_ptr(), ms, d_p.data_ptr(), d_s.data_ptr(), d_ws.data_ptr(), wsb,
                          torch.cuda.current_stream().cuda_stream, transcript=transcript, d_out_challenges=d_c.data_ptr(),
                          blind_key=blind_key, index_base=index_base, amount64=amount64)
    torch.cuda.synchronize()
    pts = d_p.cpu().numpy().view(np.uint64).reshape(npts, PW)
    off = np.concatenate([[0], np.cumsum([_nv(m, n) for m in ms])]).astype(int)
    recs = [pts[off[i]:off[i + 1]] for i in range(len(ms))]
    return recs, d_s.cpu().numpy().view(np.uint64).reshape(len(ms), 3, 4), d_p, d_s, d_c


def _verify_wire(torch, bv, d_p, d_s, ms, d_ch=None):
    wsb = bv.mixed_workspace_bytes(ms)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    d_ok = torch.full((len(ms),), 7, dtype=torch.int32, device="cuda:0")
    bv.run_mixed_device(d_p.data_ptr(), d_s.data_ptr(), ms, d_ok.data_ptr(), d_ws.data_ptr(), wsb,
                        torch.cuda.current_stream().cuda_stream, d_challenges=d_ch.data_ptr() if d_ch is not None else 0)
    torch.cuda.synchronize()
    return d_ok.cpu().tolist()


@functools.lru_cache(maxsize=None)
def _oracle_block(cname, transcript):
    """the oracle's proofs of the block against untruncated commitments, and its verdicts: [(pts, sc, V, rc)]"""
    r = _corpus(cname, N64, 1).r
    gams = _gammas(r)
    out = []
    O.set_transcript(transcript)
    try:
        for i, m in enumerate(MS):
            cp = _corpus(cname, N64, m)
            if transcript:
                O.set_blinding(O.blinding_from_key(KEY, BASE + i, _k(m, N64), r))
            Vu = _full_commitments(cp, VALS[i], gams[i])
            pts, sc, V = O.range_prove(cp.opk, N64, VALS[i], gams[i], V=Vu)
            out.append((pts, sc, V, int(O.range_verify(cp.opk, N64, m, pts, sc, V))))
    finally:
        O.set_blinding(None)
        O.set_transcript(False)
    return out


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_prove_with_the_flag_equals_the_oracle(cname):
    """(64, 2) engine, block [1, 2, 1] with amounts of 2^63 + 12345, 2^31, 2^64 - 1 and 5: every record point, scalar and V
    equals the oracle's proof against V = v g + gamma h; the verifier accepts all three; without the flag the first two are
    rejected and the third is byte-identical"""
    torch = need_gpu()
    B, a, bv = _engine(cname, N64, 2)
    gams = _gammas(_corpus(cname, N64, 1).r)
    for transcript in (False, True):
        kw = dict(transcript=True, blind_key=KEY, index_base=BASE) if transcript else {}
        recs, sc, d_p, d_s, d_c = _prove_wire(torch, bv, VALS, gams, True, **kw)
        want = _oracle_block(cname, transcript)
        for i, m in enumerate(MS):
            opts, osc, oV, orc = want[i]
            nrec = 3 + 2 * _k(m, N64)
            assert np.array_equal(recs[i][:nrec], opts), (transcript, i)
            assert np.array_equal(recs[i][nrec:], oV), (transcript, i)
            assert np.array_equal(sc[i], osc), (transcript, i)
            assert orc == 0, (transcript, i)
        assert _verify_wire(torch, bv, d_p, d_s, MS, d_c if transcript else None) == [0, 0, 0]
        recs0, sc0, d_p0, d_s0, d_c0 = _prove_wire(torch, bv, VALS, gams, False, **kw)
        assert _verify_wire(torch, bv, d_p0, d_s0, MS, d_c0 if transcript else None) == [1, 1, 0]
        assert recs0[2].tobytes() == recs[2].tobytes() and sc0[2].tobytes() == sc[2].tobytes()
        for i in (0, 1):   # the truncated commitments differ; A does not depend on them
            nrec = 3 + 2 * _k(MS[i], N64)
            assert not np.array_equal(recs0[i][nrec:], recs[i][nrec:])
            assert np.array_equal(recs0[i][0], recs[i][0])
    bv.close()


@pytest.mark.parametrize("cname,version", [("bls12_381", 1), ("bls12_381", 2), ("secp256k1", 1), ("secp256k1", 2)])
def test_bytes_with_the_flag(cname, version):
    torch = need_gpu()
    B, a, bv = _engine(cname, N64, 2)
    gams = _gammas(_corpus(cname, N64, 1).r)
    unc = version == 2
    recs, sc = _prove_wire(torch, bv, VALS, gams, True)[:2]
    for i, m in enumerate(MS):   # the wire output the bytes are compared with is the oracle's proof (the test above)
        nrec = 3 + 2 * _k(m, N64)
        assert np.array_equal(recs[i][:nrec], _oracle_block(cname, False)[i][0])
    want = b"".join(B.encode_proofs(a, N64, m, recs[i][None, :3 + 2 * _k(m, N64)], sc[i][None], version).tobytes()
                    for i, m in enumerate(MS))
    enc = B.uncompressed_points if unc else B.compress_points
    want_cm = b"".join(enc(a, recs[i][3 + 2 * _k(m, N64):]).tobytes() for i, m in enumerate(MS))
    v, g = _pack(VALS, gams)
    d_v, d_g = _dev(torch, v), _dev(torch, g)
    pb = B.uncompressed_bytes(a) if unc else B.compressed_bytes(a)
    nbytes = sum(B.proof_bytes(a, N64, m, version) for m in MS)
    d_p = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_c = torch.full((sum(MS) * pb,), 0x5a, dtype=torch.uint8, device="cuda:0")
    wsb = bv.prover_mixed_workspace_bytes(MS, serialized=True)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    bv.prove_serialized_mixed_device(d_v.data_ptr(), d_g.data_ptr(), MS, d_p.data_ptr(), d_c.data_ptr(), d_ws.data_ptr(), wsb, st,
                                     uncompressed=unc, amount64=True)
    torch.cuda.synchronize()
    assert d_p.cpu().numpy().tobytes() == want and d_c.cpu().numpy().tobytes() == want_cm
    vsb = bv.serialized_mixed_workspace_bytes(MS)
    d_vws = torch.empty(vsb, dtype=torch.uint8, device="cuda:0")
    d_ok = torch.full((len(MS),), 7, dtype=torch.int32, device="cuda:0")
    bv.verify_serialized_mixed_device(d_p.data_ptr(), d_c.data_ptr(), MS, d_ok.data_ptr(), d_vws.data_ptr(), vsb, st,
                                      uncompressed=unc)
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [0, 0, 0]
    # the host entries behind the Python wrappers: the same bytes, the same records
    hraw, hcm, hms = bv.prove_serialized_mixed(VALS, gams, uncompressed=unc, amount64=True)
    assert hraw == want and hcm == want_cm and hms.tolist() == MS
    if version == 1:
        hrecs, hsc = bv.prove_batch_mixed(VALS, gams, amount64=True)
        assert all(np.array_equal(x, y) for x, y in zip(hrecs, recs)) and np.array_equal(hsc, sc)
        # prove_batch routes to the mixed call when the flag is set: the capacity class alone
        p2, s2, V2 = bv.prove_batch([VALS[1]], [gams[1]], amount64=True)
        assert np.array_equal(np.concatenate([p2[0], V2[0]]), recs[1]) and np.array_equal(s2[0], sc[1])
    bv.close()


def test_edwards25519_against_pyref():
    torch = need_gpu()
    cname = "ed25519"
    cp = _corpus(cname, N64, 1)
    B, a, bv = _engine(cname, N64, 1)
    gam = [cp.r - 3]
    Vu = _full_commitments(cp, [BIG], gam)
    assert np.array_equal(Vu[0], O.point_to_wire(2, cp.ppk.commitment(BIG % cp.r, gam[0])))
    opts, osc, oV = cp.prove([BIG], gam, V=Vu)           # pyref with a hand-filled RangeProver
    assert np.array_equal(oV, Vu) and cp.verdict(opts, osc, oV) == 0
    recs, sc, d_p, d_s, d_c = _prove_wire(torch, bv, [[BIG]], [gam], True)
    nrec = 3 + 2 * _k(1, N64)
    assert np.array_equal(recs[0][:nrec], opts) and np.array_equal(recs[0][nrec:], oV) and np.array_equal(sc[0], osc)
    assert _verify_wire(torch, bv, d_p, d_s, [1]) == [0]
    d_p0, d_s0 = _prove_wire(torch, bv, [[BIG]], [gam], False)[2:4]
    assert _verify_wire(torch, bv, d_p0, d_s0, [1]) == [1]
    bv.close()


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_value_out_of_range_with_the_flag(cname):
    """n = 8: the flag does not widen the range.  255 verifies; 300 is the oracle's proof against V = 300 g + gamma h and is
    rejected"""
    torch = need_gpu()
    n = 8
    B, a, bv = _engine(cname, n, 4)
    r = _corpus(cname, n, 1).r
    ms = [1, 1, 2]
    vals, gams = [[255], [300], [7, 255]], [[11], [r - 2], [5, 6]]
    recs, sc, d_p, d_s, d_c = _prove_wire(torch, bv, vals, gams, True)
    want_ok = []
    for i, m in enumerate(ms):
        cp = _corpus(cname, n, m)
        opts, osc, oV = O.range_prove(cp.opk, n, vals[i], gams[i], V=_full_commitments(cp, vals[i], gams[i]))
        nrec = 3 + 2 * _k(m, n)
        assert np.array_equal(recs[i][:nrec], opts) and np.array_equal(recs[i][nrec:], oV) and np.array_equal(sc[i], osc), i
        want_ok.append(int(O.range_verify(cp.opk, n, m, opts, osc, oV)))
    assert want_ok == [0, 1, 0]
    assert _verify_wire(torch, bv, d_p, d_s, ms) == want_ok
    bv.close()


# ---- the commitment kernel -----------------------------------------------------------------------------------------------
def _amounts():
    return sorted({min(x, (1 << 64) - 1) for j in range(65) for x in (1 << j, (1 << j) - 1)})


def _gamma_set(r, seed):
    rng = random.Random(seed)
    return [0, 1, 2, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2] + [rng.randrange(r) for _ in range(8)]


COUNTS = (1, 63, 64, 65, 257)


def _inputs(r, count, seed):
    vs, gs = _amounts(), _gamma_set(r, seed)
    return [vs[i % len(vs)] for i in range(count)], [gs[i % len(gs)] for i in range(count)]


@functools.lru_cache(maxsize=None)
def _want_commitments(cname, amount64):
    """the checker's commitments of the longest run (the shorter runs are its prefixes), computed once per curve and mode:
    flags = 0 by the checker's RangeProver::commit, the flag by its point arithmetic on the whole value"""
    cp = _corpus(cname, 8, 1)
    vs, gs = _inputs(cp.r, max(COUNTS), 99 + CID[cname])
    if not amount64:
        return np.stack([cp.commit(v, g) for v, g in zip(vs, gs)])
    memo_g, memo_h = {}, {}
    out = []
    for v, g in zip(vs, gs):
        if cname != "ed25519":
            if v not in memo_g:
                memo_g[v] = O.point_mul(cp.cid, cp.gh[0], v)
            if g not in memo_h:
                memo_h[g] = O.point_mul(cp.cid, cp.gh[1], g)
            out.append(O.point_add(cp.cid, memo_g[v], memo_h[g]))
        else:
            gg, hh = cp.ppk.g, cp.ppk.h
            if v not in memo_g:
                memo_g[v] = cp.grp.mul(gg, v % cp.r)
            if g not in memo_h:
                memo_h[g] = cp.grp.mul(hh, g)
            out.append(O.point_to_wire(2, cp.grp.add(memo_g[v], memo_h[g])))
    return np.stack(out)


def _commit_device(torch, bv, vs, gs, amount64):
    """-> (count, PW) points; the buffer is one point longer and that point must come back untouched"""
    count, PW = len(vs), bv.arith.PW
    d_v = _dev(torch, np.array(vs, dtype=np.uint64))
    d_g = _dev(torch, O.scalars_to_wire(gs))
    d_o = torch.full(((count + 1) * PW * 8,), 0x5a, dtype=torch.uint8, device="cuda:0")
    bv.commit_batch_device(d_v.data_ptr(), d_g.data_ptr(), count, d_o.data_ptr(), torch.cuda.current_stream().cuda_stream,
                           amount64=amount64)
    torch.cuda.synchronize()
    out = d_o.cpu().numpy().view(np.uint64).reshape(count + 1, PW)
    assert (out[count] == 0x5a5a5a5a5a5a5a5a).all(), "the kernel wrote past its last commitment"
    return out[:count]


@pytest.mark.parametrize("window_bits", (5, 13))
@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1", "ed25519"))
def test_commit_kernel(cname, window_bits):
    torch = need_gpu()
    cp = _corpus(cname, 8, 1)
    B, a, bv = _engine(cname, 8, 1, window_bits)
    r, PW = cp.r, a.PW
    inf = np.zeros(PW, dtype=np.uint64)
    inf[PW - 1] = 1
    for amount64 in (False, True):
        want = _want_commitments(cname, amount64)
        for count in COUNTS:
            vs, gs = _inputs(r, count, 99 + CID[cname])
            got = _commit_device(torch, bv, vs, gs, amount64)
            bad = [i for i in range(count) if not np.array_equal(got[i], want[i])]
            assert not bad, (amount64, count, bad[:5], [hex(vs[i]) for i in bad[:5]])
        # PublicKey::new has h = 2 g: the identity, P + P and P - P inside the walk
        assert np.array_equal(O.point_mul(cp.cid, cp.gh[0], 2) if cname != "ed25519" else
                              O.point_to_wire(2, cp.grp.mul(cp.ppk.g, 2)), cp.gh[1])
        pins = _commit_device(torch, bv, [0, 2, 2], [0, 1, r - 1], amount64)
        assert np.array_equal(pins[0], inf) and np.array_equal(pins[2], inf)
        assert np.array_equal(pins[1], _mul_add(cp, cp.gh, 4, 0))
        assert not np.array_equal(pins[1], inf)
        # the host entry, and for the same (v, gamma) the commitments the mixed prove call forms under the same flag
        vs, gs = _inputs(r, max(COUNTS), 99 + CID[cname])
        assert np.array_equal(bv.commit_batch(vs[:65], gs[:65], amount64=amount64), want[:65])
        pick = [0, 2, 3, 62, 63, 64] + [vs.index(1 << 31), vs.index((1 << 64) - 1)]
        pv, pg = [vs[i] for i in pick] + [0, 2, 2], [gs[i] for i in pick] + [0, 1, r - 1]
        recs, _ = bv.prove_batch_mixed([[v] for v in pv], [[g] for g in pg], amount64=amount64)
        got = bv.commit_batch(pv, pg, amount64=amount64)
        for j in range(len(pv)):
            assert np.array_equal(recs[j][-1], got[j]), (amount64, j)
    bv.close()


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1", "ed25519"))
def test_commit_kernel_on_a_hashed_key(cname):
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cp = _corpus(cname, 8, 1)
    a = B.Arith(cname)
    pk = B.PublicKey.hashed(a, 8, b"amount64 test key")
    bv = B.BatchVerifier(pk, 8, 1, window_bits=5)
    rng = random.Random(4242 + CID[cname])
    vs = [rng.randrange(1 << 64) for _ in range(40)] + [rng.randrange(1 << 31) for _ in range(8)]
    gs = [rng.randrange(cp.r) for _ in vs]
    for amount64 in (False, True):
        got = _commit_device(torch, bv, vs, gs, amount64)
        for i, (v, g) in enumerate(zip(vs, gs)):
            assert np.array_equal(got[i], _mul_add(cp, pk.gh, v if amount64 else _i32(v), g)), (amount64, i)
    bv.close()


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1", "ed25519"))
def test_mirror_commitment_is_the_provers_point(cname):
    """RangeProver.commit(amount64=True) forms V as a two-term MulVec (bpp_msm).  bpp_range_prove compares the caller's V
    with the batch prover's by bytes, so the MulVec must give the very wire point -- on ristretto255 the same
    representative -- that the prover and the commit kernel write, and that the checker computes"""
    need_gpu()
    B, a, bv = _engine(cname, 8, 1)
    cp = _corpus(cname, 8, 1)
    pk = B.PublicKey.from_points(a, cp.gh, cp.G, cp.H)
    vs = [BIG, 1 << 31, (1 << 64) - 1, 5, 0, 2, 2]
    gs = [cp.r - 3, 77, (cp.r - 1) // 2, 9, 0, 1, cp.r - 1]
    pr = B.RangeProver.new()
    for v, g in zip(vs, gs):
        pr.commit(pk, v, g, amount64=True)
    got = bv.commit_batch(vs, gs, amount64=True)
    recs, _ = bv.prove_batch_mixed([[v] for v in vs], [[g] for g in gs], amount64=True)
    for j, (v, g) in enumerate(zip(vs, gs)):
        assert pr.commitment_vec[j].tobytes() == got[j].tobytes() == recs[j][-1].tobytes(), j
        assert np.array_equal(got[j], _mul_add(cp, cp.gh, v, g)), j
    bv.close()


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1", "ed25519"))
def test_commit_host_twin_at_one_amount_and_a_few(cname):
    """bpp_commit_batch on host pointers at count 1 and 5, with and without the flag, against the checker's v g + gamma h"""
    need_gpu()
    B, a, bv = _engine(cname, 8, 1)
    cp = _corpus(cname, 8, 1)
    vs, gs = [BIG, 5, (1 << 64) - 1, 0, 1 << 31], [cp.r - 3, 9, 77, 0, (cp.r - 1) // 2]
    for count in (1, 5):
        for amount64 in (False, True):
            got = bv.commit_batch(vs[:count], gs[:count], amount64=amount64)
            assert got.shape[0] == count
            for j in range(count):
                assert np.array_equal(got[j], _mul_add(cp, cp.gh, vs[j] if amount64 else _i32(vs[j]), gs[j])), (count, amount64, j)
    bv.close()


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_single_call_takes_untruncated_commitments(cname):
    """RangeProof.prove with hand-made untruncated commitments: the first call with a key (no engine yet), the second (the
    engine is built: the batch prover in amount mode), the fourth, and with the cache off (the fold-based prover) all give
    the oracle's proof.  The outputs are the same on every path by construction, so which path ran is told by time alone:
    tools/amount_bench.py records it (leg `single`)"""
    need_gpu()
    import bulletproofsplus_amd as B
    cp = _corpus(cname, N64, 1)
    a = B.Arith(cname)
    pk = B.PublicKey.from_points(a, cp.gh, cp.G, cp.H)
    gam = _gammas(cp.r)[0]
    opts, osc, oV, orc = _oracle_block(cname, False)[0]
    assert orc == 0

    def prove():
        pr = B.RangeProver.new()
        pr.v_vec, pr.gamma_vec, pr.commitment_vec = [BIG], [B.api.scalar_to_wire(gam[0])], [oV[0]]
        pf = B.RangeProof.prove(pk, N64, pr)
        assert np.array_equal(pf.points_wire(), opts) and np.array_equal(pf.scalars_wire(), osc)
        pf.verify(pk, N64, oV)
        return pf

    for _ in range(4):
        prove()
    a.set_verify_cache(False)
    try:
        prove()
    finally:
        a.set_verify_cache(True)
    # the reference's own commitment still takes the first attempt: byte-identical to the oracle's truncating proof
    pr = B.RangeProver.new()
    pr.commit(pk, 5, 9)
    prove()   # (the key's engine exists again)
    pf = B.RangeProof.prove(pk, N64, pr)
    tp, ts, tV = O.range_prove(cp.opk, N64, [5], [9])
    assert np.array_equal(pf.points_wire(), tp) and np.array_equal(pf.scalars_wire(), ts) and np.array_equal(pr.commitment_vec[0], tV[0])
