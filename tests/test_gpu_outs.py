"""-m gpu: proofs over ANY number of outputs (the *_outs* entries; csrc/outs_plan.hpp, include/bpp_amd.h "proofs over ANY
number of outputs").  A proof over o outputs is the proof of shape (n, M), M = 2^ceil(log2 o), over its values and masks
padded with zeros; the streams carry the real outputs alone.

Expected values never come from the library.  Containers and commitments are the oracle's prover on the zero-padded shapes
(the C oracle, edwards25519: pyref), encoded by pyref.  Verdicts are the CHECKER's on the padded statement
[V_0 .. V_{o-1}, identity x (M - o)], 2 for a container the test damaged.  Masks, pads and tags are hashlib's
(output_cases); the hit list and the candidate count are built from those over the REAL outputs only.  The three checks
that run existing calls beside the new ones say so: library against library."""

import functools
import hashlib
import random

import numpy as np
import pytest

import oracle as O
import output_cases as OC
import pyref as P
import recover_cases as RC
import test_gpu_find as TF
import test_gpu_recover as TR
import verdict_corpus as VC
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

CID, CURVES, N, BASE = TR.CID, TR.CURVES, TR.N, TR.BASE
CAP = 8
GUARD = TF.GUARD
FORMS = [(c, 1) for c in CURVES] + [("bls12_381", 2), ("secp256k1", 2)]
# every count 1..8; class 4: six proofs of 17 record points, 102 lanes; class 8: five of 23, 115 lanes -- both cross a wave
OUTS = [3, 1, 8, 5, 2, 3, 7, 4, 6, 3, 3, 5, 1, 3]
SHAPES = [1 << (o - 1).bit_length() for o in OUTS]
FIRST = [sum(OUTS[:i]) for i in range(len(OUTS))]
N_OUT = sum(OUTS)
PROOF_OF = [i for i, o in enumerate(OUTS) for _ in range(o)]
PLACE_OF = [j for o in OUTS for j in range(o)]
BIG = (0, 1)   # proof 0 (three outputs), place 1: an amount of 2^31 and more
TAMPERED, DAMAGED, HALVED, SWAPPED = 6, 9, 3, 10
assert SHAPES == [4, 1, 8, 8, 2, 4, 8, 4, 8, 4, 4, 8, 1, 4] and N_OUT == 54 and sorted(set(OUTS)) == list(range(1, 9))
assert SHAPES.count(4) * 17 == 102 and SHAPES.count(8) * 23 == 115


def _k(m):
    return TR._k(N, m)


def _values(cname):
    r = RC.ORDER[cname]
    rng = random.Random(9100 + CID[cname])
    vals = [[rng.randrange(1 << N) for _ in range(o)] for o in OUTS]
    gams = [[rng.randrange(1, r) for _ in range(o)] for o in OUTS]
    vals[BIG[0]][BIG[1]] = (1 << 31) + 77
    return vals, gams


def _pad(xs, m):
    return list(xs) + [0] * (m - len(xs))


class _Transcript:
    """the checker under the transcript (literal blinding), or under the literals"""

    def __init__(self, cp, on):
        self.cp, self.on = cp, on

    def __enter__(self):
        if not self.on:
            return
        if self.cp.cname == "ed25519":
            P.Transcript.fs = P.FsTranscript(self.cp.curve, 2, self.cp.n, self.cp.m, self.cp.ppk)
        else:
            O.set_transcript(True)

    def __exit__(self, *exc):
        if not self.on:
            return
        if self.cp.cname == "ed25519":
            P.Transcript.fs = None
        else:
            O.set_transcript(False)


@functools.lru_cache(maxsize=None)
def _oracle_proof(cname, transcript, full, i):
    """the oracle's proof of proof i on its zero-padded shape -> (pts, sc, V); full: against V = v g + gamma h over the whole
    u64 (BPP_PROVE_AMOUNT64) -- for amounts below 2^31 that is the same proof, and the cache knows"""
    vals, gams = _values(cname)
    m = SHAPES[i]
    cp = TR._corpus(cname, N, m)
    v, g = _pad(vals[i], m), _pad(gams[i], m)
    V = None
    if full:
        from test_gpu_amount64 import _full_commitments
        V = _full_commitments(cp, v, g)
    with _Transcript(cp, transcript):
        pts, sc, V = cp.prove(v, g, V=V)
    # the padded commitments of the definition are the identity
    assert all(int(w[2 * cp.L]) == 1 for w in V[OUTS[i]:]) and all(int(w[2 * cp.L]) == 0 for w in V[:OUTS[i]])
    return pts, sc, V


def _oracle(cname, transcript, amount64, i):
    vals, _ = _values(cname)
    return _oracle_proof(cname, transcript, bool(amount64 and max(vals[i]) >= 1 << 31), i)


@functools.lru_cache(maxsize=None)
def _verdict(cname, transcript, amount64, i, defect=None):
    """the checker on the padded statement of proof i, with the defect the test put into it"""
    pts, sc, V = _oracle(cname, transcript, amount64, i)
    cp = TR._corpus(cname, N, SHAPES[i])
    sc, V = sc.copy(), V.copy()
    if defect == "tampered":
        sc[0] = O.scalars_to_wire([(O.limbs_to_int(sc[0]) + 1) % cp.r])[0]
    if defect == "swapped":
        V[1] = _oracle(cname, transcript, amount64, 0)[2][0]
    if isinstance(defect, tuple):   # ("drop", j): V_j presented as the identity
        V[defect[1]] = 0
        V[defect[1]][2 * cp.L] = 1
    with _Transcript(cp, transcript):
        return cp.verdict(pts, sc, V)


def _encoded(cname, transcript, amount64, version):
    """pyref's bytes of the oracle's block -> (containers per proof, real commitments per proof, padded ones per proof)"""
    blobs, real, padded = [], [], []
    for i, o in enumerate(OUTS):
        cp = TR._corpus(cname, N, SHAPES[i])
        pts, sc, V = _oracle(cname, transcript, amount64, i)
        blob, comm = VC.encode_case(cp, VC.Case("p", pts, sc, V), version)
        pb = len(comm) // SHAPES[i]
        blobs.append(blob)
        real.append(comm[:o * pb])
        padded.append(comm[o * pb:])
    return blobs, real, padded


def _identity_bytes(cname, version):
    return {("bls12_381", 1): b"\xc0" + bytes(47), ("bls12_381", 2): b"\x40" + bytes(95), ("secp256k1", 1): bytes(33),
            ("secp256k1", 2): bytes(65), ("ed25519", 1): bytes(32)}[cname, version]


_engines = {}


def _engine(cname):
    if cname not in _engines:
        _engines[cname] = TR._engine(cname, cap=CAP)
    return _engines[cname]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for _, _, bv in _engines.values():
        bv.close()
    _engines.clear()


def _split(B, a, raw, cm, version, outs=OUTS):
    pb = B.uncompressed_bytes(a) if version == 2 else B.compressed_bytes(a)
    shapes = [1 << (o - 1).bit_length() for o in outs]
    po = np.concatenate([[0], np.cumsum([B.proof_bytes(a, N, m, version) for m in shapes])]).astype(int)
    co = np.concatenate([[0], np.cumsum([o * pb for o in outs])]).astype(int)
    assert len(raw) == po[-1] and len(cm) == co[-1]
    return [bytes(raw[po[i]:po[i + 1]]) for i in range(len(outs))], [bytes(cm[co[i]:co[i + 1]]) for i in range(len(outs))]


def _verify_device(torch, bv, raw, cm, outs, transcript, version, group=None):
    dev = torch.device("cuda:0")
    d_p = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    d_c = torch.frombuffer(bytearray(cm), dtype=torch.uint8).to(dev)
    d_ok = TR._dev(torch, np.full(len(outs) + 2, GUARD, dtype=np.uint32))
    wsb = bv.serialized_outs_workspace_bytes(outs, group)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    bv.verify_serialized_outputs_device(d_p.data_ptr(), d_c.data_ptr(), outs, d_ok.data_ptr() + 4, d_ws.data_ptr(), wsb,
                                        torch.cuda.current_stream().cuda_stream, transcript=transcript,
                                        uncompressed=version == 2, group=group, weight_key=hashlib.sha256(b"w").digest())
    torch.cuda.synchronize()
    ok = d_ok.cpu().numpy().view(np.uint32).tolist()
    assert ok[0] == ok[-1] == GUARD
    return ok[1:-1]


# ---- 1. the prover against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("amount64", (False, True))
@pytest.mark.parametrize("transcript", (False, True))
@pytest.mark.parametrize("cname,version", FORMS)
def test_prover_is_the_oracle_on_the_padded_shapes(cname, version, transcript, amount64):
    """containers and the sum(outs) commitment encodings equal the oracle's prover on the zero-padded shapes, under the
    literals and under the transcript with literal blinding, with and without BPP_PROVE_AMOUNT64 (one amount of 2^31 + 77
    at a real place); the device entry between guard bytes gives the same bytes"""
    torch = need_gpu()
    B, a, bv = _engine(cname)
    vals, gams = _values(cname)
    blobs, real, padded = _encoded(cname, transcript, amount64, version)
    assert all(p == _identity_bytes(cname, version) * (m - o) for p, m, o in zip(padded, SHAPES, OUTS))
    raw, cm, outs = bv.prove_serialized_outputs(vals, gams, transcript=transcript, uncompressed=version == 2, amount64=amount64)
    assert outs.tolist() == OUTS
    pr, cs = _split(B, a, raw, cm, version)
    for i in range(len(OUTS)):
        assert pr[i] == blobs[i], (i, OUTS[i])
        assert cs[i] == real[i], (i, OUTS[i])
    assert B.proofs_scan(a, N, raw, version).tolist() == SHAPES and B.outs_shapes(OUTS, CAP).tolist() == SHAPES
    # the device entry: the same bytes, nothing beyond them
    v = np.array([x for row in vals for x in row], dtype=np.uint64)
    g = O.scalars_to_wire([x for row in gams for x in row])
    d_v, d_g = TR._dev(torch, v), TR._dev(torch, g)
    d_p = torch.full((len(raw) + 16,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_c = torch.full((len(cm) + 16,), 0x5a, dtype=torch.uint8, device="cuda:0")
    wsb = bv.prover_serialized_outs_workspace_bytes(OUTS)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    bv.prove_serialized_outputs_device(d_v.data_ptr(), d_g.data_ptr(), OUTS, d_p.data_ptr() + 8, d_c.data_ptr() + 8, d_ws.data_ptr(),
                                       wsb, torch.cuda.current_stream().cuda_stream, transcript=transcript,
                                       uncompressed=version == 2, amount64=amount64)
    torch.cuda.synchronize()
    assert d_p.cpu().numpy().tobytes() == b"\x5a" * 8 + raw + b"\x5a" * 8
    assert d_c.cpu().numpy().tobytes() == b"\x5a" * 8 + cm + b"\x5a" * 8


# ---- 2. verdicts against the checker ---------------------------------------------------------------------------------------
def _defective(cname, transcript, version):
    """the oracle's block with four defects -> (containers, commitments, the checker's verdicts)"""
    blobs, real, _ = _encoded(cname, transcript, False, version)
    blobs, real = list(blobs), list(real)
    r = RC.ORDER[cname]
    t = bytearray(blobs[TAMPERED])
    tail = len(t) - 96
    t[tail:tail + 32] = ((int.from_bytes(t[tail:tail + 32], "little") + 1) % r).to_bytes(32, "little")
    blobs[TAMPERED] = bytes(t)
    d = bytearray(blobs[DAMAGED])
    d[9] ^= 1   # a reserved byte
    blobs[DAMAGED] = bytes(d)
    h = bytearray(blobs[HALVED])
    assert h[7] == SHAPES[HALVED] == 8
    h[7] = 4
    blobs[HALVED] = bytes(h)
    pb = len(real[0]) // OUTS[0]
    s = bytearray(real[SWAPPED])
    s[pb:2 * pb] = real[0][:pb]
    real[SWAPPED] = bytes(s)
    defect = {TAMPERED: "tampered", SWAPPED: "swapped"}
    want = [2 if i in (DAMAGED, HALVED) else _verdict(cname, transcript, False, i, defect.get(i)) for i in range(len(OUTS))]
    return blobs, real, want


@pytest.mark.parametrize("transcript", (False, True))
@pytest.mark.parametrize("cname,version", FORMS)
def test_verdicts_are_the_checkers(cname, version, transcript):
    """one container tampered (r' + 1): 1; one damaged header byte: 2; one header m halved: 2 for that proof only; one real
    commitment replaced by another valid point: 1 -- through the exact call, the grouped call (group = 4) and the host twins"""
    torch = need_gpu()
    B, a, bv = _engine(cname)
    blobs, real, want = _defective(cname, transcript, version)
    assert want[TAMPERED] == 1 and want[SWAPPED] == 1 and want[DAMAGED] == want[HALVED] == 2
    clean = [_verdict(cname, transcript, False, i) for i in range(len(OUTS))]
    assert [w for i, w in enumerate(want) if i not in (TAMPERED, DAMAGED, HALVED, SWAPPED)] == \
           [w for i, w in enumerate(clean) if i not in (TAMPERED, DAMAGED, HALVED, SWAPPED)]
    assert 0 in want   # the big amount is out of range at n = 8: proof 0 is the checker's to judge, the others verify
    raw, cm = b"".join(blobs), b"".join(real)
    unc = version == 2
    assert bv.verify_serialized_outputs(raw, cm, OUTS, transcript=transcript, uncompressed=unc).tolist() == want
    assert bv.verify_serialized_outputs(raw, cm, OUTS, transcript=transcript, uncompressed=unc, group=4).tolist() == want
    assert _verify_device(torch, bv, raw, cm, OUTS, transcript, version) == want
    assert _verify_device(torch, bv, raw, cm, OUTS, transcript, version, group=4) == want
    # the untouched block: the checker's verdicts of the oracle's proofs
    blobs0, real0, _ = _encoded(cname, transcript, False, version)
    assert _verify_device(torch, bv, b"".join(blobs0), b"".join(real0), OUTS, transcript, version) == clean


# ---- 3. soundness of the padding ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transcript", (False, True))
@pytest.mark.parametrize("cname", CURVES)
def test_a_real_fourth_output_is_not_padding(cname, transcript):
    """a proof made over four real outputs (V_3 = 1 g + 0 h), presented as outs = 3 with its first three commitments, gets
    1; the same container with outs = 4 and all four commitments gets 0"""
    need_gpu()
    B, a, bv = _engine(cname)
    cp = TR._corpus(cname, N, 4)
    vals, gams = [[5, 200, 7, 1]], [[11, 12, 13, 0]]
    with _Transcript(cp, transcript):
        pts, sc, V = cp.prove(vals[0], gams[0])
        Vdrop = V.copy()
        Vdrop[3] = 0
        Vdrop[3][2 * cp.L] = 1
        want4, want3 = cp.verdict(pts, sc, V), cp.verdict(pts, sc, Vdrop)
    assert (want4, want3) == (0, 1)
    blob, comm = VC.encode_case(cp, VC.Case("p", pts, sc, V), 1)
    raw, cm, outs = bv.prove_serialized_outputs(vals, gams, transcript=transcript)
    assert outs.tolist() == [4] and raw == blob and cm == comm
    pb = len(cm) // 4
    assert bv.verify_serialized_outputs(raw, cm, [4], transcript=transcript).tolist() == [0]
    assert bv.verify_serialized_outputs(raw, cm[:3 * pb], [3], transcript=transcript).tolist() == [1]
    # ... and the honest three-output proof of the same first three amounts verifies as three
    raw3, cm3, _ = bv.prove_serialized_outputs([vals[0][:3]], [gams[0][:3]], transcript=transcript)
    assert cm3 == cm[:3 * pb] and raw3 != raw
    assert bv.verify_serialized_outputs(raw3, cm3, [3], transcript=transcript).tolist() == [0]


# ---- 4. compatibility with the existing calls: library against library ----------------------------------------------------
@pytest.mark.parametrize("cname,version", FORMS)
def test_existing_calls_agree_on_the_padded_block(cname, version):
    """LIBRARY AGAINST LIBRARY.  The containers with the identity encodings appended verify through verify_serialized_mixed
    with ms = M; prove_serialized_mixed on the zero-padded inputs gives the same container bytes; verify_wire_mixed accepts
    the oracle's records with the canonical infinity in the padded slots"""
    need_gpu()
    B, a, bv = _engine(cname)
    vals, gams = _values(cname)
    unc = version == 2
    ident = _identity_bytes(cname, version)
    for transcript in (False, True):
        raw, cm, _ = bv.prove_serialized_outputs(vals, gams, transcript=transcript, uncompressed=unc)
        pr, cs = _split(B, a, raw, cm, version)
        padded_cm = b"".join(c + ident * (m - o) for c, m, o in zip(cs, SHAPES, OUTS))
        want = [_verdict(cname, transcript, False, i) for i in range(len(OUTS))]
        assert bv.verify_serialized_mixed(raw, padded_cm, SHAPES, transcript=transcript, uncompressed=unc).tolist() == want
        assert bv.verify_serialized_outputs(raw, cm, OUTS, transcript=transcript, uncompressed=unc).tolist() == want
        pv = [_pad(v, m) for v, m in zip(vals, SHAPES)]
        pg = [_pad(g, m) for g, m in zip(gams, SHAPES)]
        raw2, cm2, ms2 = bv.prove_serialized_mixed(pv, pg, transcript=transcript, uncompressed=unc)
        assert ms2.tolist() == SHAPES and raw2 == raw and cm2 == padded_cm
        if version == 1:
            recs = [np.concatenate([x[0], x[2]]) for x in (_oracle(cname, transcript, False, i) for i in range(len(OUTS)))]
            scs = np.stack([_oracle(cname, transcript, False, i)[1] for i in range(len(OUTS))])
            if not transcript:   # the wire call draws no challenges: the literals
                assert bv.verify_wire_mixed(recs, scs, SHAPES).tolist() == want


# ---- 5. the output finder -------------------------------------------------------------------------------------------------
K0 = hashlib.sha256(b"outs: scanning key 0").digest()
K1 = hashlib.sha256(b"outs: scanning key 1").digest()
FOREIGN = hashlib.sha256(b"outs: a key nobody scans with").digest()
SENDER = hashlib.sha256(b"outs: the sender's blinding key").digest()
OWNER = [[K0, K1, FOREIGN][(5 * o + o // 7) % 3] for o in range(N_OUT)]
OWNER[FIRST[1]] = FOREIGN          # proof 1's only output: the byte behind proof 0's three
OVERRUN = (0, 3)                   # proof 0 has three outputs: its place 3 is padding
F_TAMPERED, F_DAMAGED = 5, 8


def _find_key2():
    """a third scanning key whose tag for the PADDED place (0, 3) equals the tag byte of the next proof's output 0 -- the
    byte an unmasked lane would read at first + 3: a hashlib search"""
    want = OC.tag(OWNER[FIRST[1]], BASE + 1, 0)
    for t in range(1 << 16):
        k = hashlib.sha256(b"outs: scanning key 2, try %d" % t).digest()
        if OC.tag(k, BASE + OVERRUN[0], OVERRUN[1]) == want and OC.tag(k, BASE + 1, 0) != want:
            return k
    raise AssertionError("no key found")


K2 = _find_key2()
KEYS = [K0, K1, K2]
assert OUTS[OVERRUN[0]] == OVERRUN[1] and FIRST[OVERRUN[0]] + OVERRUN[1] == FIRST[1]

_find_blocks = {}


def _find_block(cname, version):
    if (cname, version) in _find_blocks:
        return _find_blocks[cname, version]
    r = RC.ORDER[cname]
    B, a, bv = _engine(cname)
    rng = random.Random(9200 + CID[cname])
    amounts = [rng.randrange(1 << N) for _ in range(N_OUT)]
    idx = [BASE + PROOF_OF[o] for o in range(N_OUT)]
    masks = [OC.mask(OWNER[o], idx[o], PLACE_OF[o], r) for o in range(N_OUT)]
    sealed = [amounts[o] ^ OC.pad(OWNER[o], idx[o], PLACE_OF[o]) for o in range(N_OUT)]
    tags = [OC.tag(OWNER[o], idx[o], PLACE_OF[o]) for o in range(N_OUT)]
    lm, ls, lt = bv.make_outputs(OWNER, amounts, OUTS, index_base=BASE)   # per output, j < outs: no ragged form needed
    assert [int.from_bytes(np.ascontiguousarray(x).tobytes(), "little") for x in lm] == masks
    assert ls.tolist() == sealed and lt.tolist() == tags
    vals = [[amounts[FIRST[i] + j] for j in range(o)] for i, o in enumerate(OUTS)]
    gm = [[masks[FIRST[i] + j] for j in range(o)] for i, o in enumerate(OUTS)]
    kw = dict(transcript=True, blind_key=SENDER, index_base=BASE)
    raw, cm, outs = bv.prove_serialized_outputs(vals, gm, uncompressed=version == 2, **kw)
    # the wire records of the same proofs, for the checker: the padded shapes through the existing prover
    recs, sc = bv.prove_batch_mixed([_pad(v, m) for v, m in zip(vals, SHAPES)], [_pad(g, m) for g, m in zip(gm, SHAPES)], **kw)
    recs, sc = list(recs), [np.array(x) for x in sc]
    pr, cs = _split(B, a, raw, cm, version)
    t = bytearray(pr[F_TAMPERED])
    tail = len(t) - 96
    rp1 = (int.from_bytes(t[tail:tail + 32], "little") + 1) % r
    t[tail:tail + 32] = rp1.to_bytes(32, "little")
    pr[F_TAMPERED] = bytes(t)
    sc[F_TAMPERED][0] = O.scalars_to_wire([rp1])[0]
    bad = bytearray(pr[F_DAMAGED])
    bad[7] ^= 3   # the header's m
    pr[F_DAMAGED] = bytes(bad)
    verdict = [2 if i == F_DAMAGED else TF._checker_verdict(cname, m, recs[i], sc[i]) for i, m in enumerate(SHAPES)]
    assert verdict == [1 if i == F_TAMPERED else 2 if i == F_DAMAGED else 0 for i in range(len(OUTS))]
    hits = [(q, o, amounts[o], masks[o]) for q, k in enumerate(KEYS) for o in range(N_OUT)
            if OWNER[o] == k and verdict[PROOF_OF[o]] == 0]
    cands = [(q, o) for q, k in enumerate(KEYS) for o in range(N_OUT)
             if verdict[PROOF_OF[o]] == 0 and OC.tag(k, idx[o], PLACE_OF[o]) == tags[o]]
    blk = dict(B=B, bv=bv, raw=b"".join(pr), cm=b"".join(cs), sealed=sealed, tags=tags, verdict=verdict, hits=hits, cands=cands)
    _find_blocks[cname, version] = blk
    return blk


def _find_device(torch, bv, raw, cm, outs, keys, sealed, tags, max_hits, version=1):
    count, nk = len(outs), len(keys)
    dev = torch.device("cuda:0")
    d_p = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    d_c = torch.frombuffer(bytearray(cm), dtype=torch.uint8).to(dev)
    d_k = torch.frombuffer(bytearray(b"".join(keys) or bytes(32)), dtype=torch.uint8).to(dev)
    d_s = TR._dev(torch, np.array(sealed, dtype=np.uint64))
    d_t = TR._dev(torch, np.array(tags, dtype=np.uint8))
    d_ok = TR._dev(torch, np.full(count + 2, GUARD, dtype=np.uint32))
    d_hits = TR._dev(torch, np.full((max_hits + 3) * 12, GUARD, dtype=np.uint32))
    d_n = TR._dev(torch, np.full(4, GUARD, dtype=np.uint32))   # [n_hits, guard, n_candidates, guard]
    wsb = bv.verify_find_outputs_outs_workspace_bytes(outs, nk)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    bv.verify_find_outputs_serialized_outs_keys_device(d_p.data_ptr(), d_c.data_ptr(), outs, d_k.data_ptr() if nk else 0, nk,
                                                       d_s.data_ptr(), d_t.data_ptr(), d_ok.data_ptr() + 4, d_hits.data_ptr(),
                                                       max_hits, d_n.data_ptr(), d_ws.data_ptr(), wsb,
                                                       torch.cuda.current_stream().cuda_stream, uncompressed=version == 2,
                                                       index_base=BASE, d_n_candidates=d_n.data_ptr() + 8)
    torch.cuda.synchronize()
    n = d_n.cpu().numpy().view(np.uint32).tolist()
    ok = d_ok.cpu().numpy().view(np.uint32).tolist()
    assert n[1] == n[3] == GUARD and ok[0] == ok[-1] == GUARD
    return ok[1:-1], d_hits.cpu().numpy().view(np.uint32).reshape(-1, 12), n[0], n[2]


def _records(hits):
    out = []
    for q, o, amount, mask in hits:
        out.append([q, o, amount & 0xffffffff, amount >> 32] + [(mask >> (32 * t)) & 0xffffffff for t in range(8)])
    return out


@pytest.mark.parametrize("cname,version", FORMS)
def test_finder_lists_real_outputs_only(cname, version):
    """54 real outputs under three scanning keys and one foreign key: hits and their order, amounts, masks and the candidate
    count are hashlib's over the real outputs; max_hits below the hit count still counts them all; the overrun byte (the
    next proof's first tag, matched by K2 at the padded place (0, 3)) is no candidate; with no keys the verdicts remain"""
    torch = need_gpu()
    blk = _find_block(cname, version)
    bv, hits, cands, verdict = blk["bv"], blk["hits"], blk["cands"], blk["verdict"]
    assert len(hits) > 20 and {q for q, *_ in hits} == {0, 1} and len(cands) >= len(hits)
    # what an unmasked lane would have counted: K2 at the padded place of proof 0 against the byte at first + 3
    assert OC.tag(K2, BASE + OVERRUN[0], OVERRUN[1]) == blk["tags"][FIRST[OVERRUN[0]] + OVERRUN[1]]
    assert (2, FIRST[1]) not in cands and verdict[0] == 0 and verdict[1] == 0
    unc = version == 2
    ok, got, found, n_cand = bv.verify_find_outputs_serialized_outs_keys(blk["raw"], blk["cm"], OUTS, KEYS, blk["sealed"], blk["tags"],
                                                                         uncompressed=unc, index_base=BASE)
    assert ok.tolist() == verdict
    assert got == hits   # K2 owns nothing: its candidates are chance, and the overrun byte is none
    assert found == len(hits) and n_cand == len(cands)
    assert all(o < N_OUT for _, o, _, _ in got)
    # the device entry between guard words; fewer records than hits: all counted, the first ones listed
    for max_hits in (len(hits) + 2, 5):
        ok, rec, found, n_cand = _find_device(torch, bv, blk["raw"], blk["cm"], OUTS, KEYS, blk["sealed"], blk["tags"], max_hits, version)
        assert ok == verdict and found == len(hits) and n_cand == len(cands)
        keep = min(max_hits, len(hits))
        assert rec[:keep].tolist() == _records(hits[:keep])
        assert (rec[keep:] == GUARD).all()
    # no hit of K2 may carry an output of proof 1 that is not its own pair; K2 alone: its candidates are hashlib's
    ok, rec, found, n_cand = _find_device(torch, bv, blk["raw"], blk["cm"], OUTS, [K2], blk["sealed"], blk["tags"], 8, version)
    assert ok == verdict and found == 0 and n_cand == len([c for c in cands if c[0] == 2])
    # without keys: the verdicts of the verify call, no hit, no candidate
    ok, rec, found, n_cand = _find_device(torch, bv, blk["raw"], blk["cm"], OUTS, [], blk["sealed"], blk["tags"], 4, version)
    assert ok == verdict and found == 0 and n_cand == 0 and (rec == GUARD).all()
    assert bv.verify_serialized_outputs(blk["raw"], blk["cm"], OUTS, transcript=True, uncompressed=unc).tolist() == verdict


# ---- 6. argument errors on a live engine ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_counts_the_engine_does_not_take(cname):
    """outs = 0 and outs = 9 on the (8, 8) engine: BPP_E_ARG naming the index, nothing written -- guard words around d_ok
    and the hit buffer intact -- and every size getter answers 0"""
    torch = need_gpu()
    B, a, bv = _engine(cname)
    blk = _find_block(cname, 1)
    for bad in (0, CAP + 1):
        outs = list(OUTS)
        outs[4] = bad
        assert bv.serialized_outs_workspace_bytes(outs) == 0 and bv.serialized_outs_workspace_bytes(outs, 4) == 0
        assert bv.prover_serialized_outs_workspace_bytes(outs) == 0 and bv.verify_find_outputs_outs_workspace_bytes(outs, 3) == 0
        with pytest.raises(B.BppError) as ei:
            B.outs_shapes(outs, CAP)
        assert ei.value.code == -1 and "outs_of[4] = %d" % bad in str(ei.value)
        dev = torch.device("cuda:0")
        d_buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)   # proofs, commitments, keys, sealed, tags: never read
        d_ok = TR._dev(torch, np.full(len(outs) + 2, GUARD, dtype=np.uint32))
        d_hits = TR._dev(torch, np.full(8 * 12, GUARD, dtype=np.uint32))
        d_n = TR._dev(torch, np.full(4, GUARD, dtype=np.uint32))
        d_ws = torch.full((1 << 20,), 0x5a, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        calls = (
            lambda: bv.verify_serialized_outputs_device(d_buf.data_ptr(), d_buf.data_ptr(), outs, d_ok.data_ptr() + 4, d_ws.data_ptr(),
                                                        1 << 20, st, transcript=True),
            lambda: bv.verify_serialized_outputs_device(d_buf.data_ptr(), d_buf.data_ptr(), outs, d_ok.data_ptr() + 4, d_ws.data_ptr(),
                                                        1 << 20, st, transcript=True, group=4, weight_key=bytes(32)),
            lambda: bv.verify_find_outputs_serialized_outs_keys_device(
                d_buf.data_ptr(), d_buf.data_ptr(), outs, d_buf.data_ptr(), 3, d_buf.data_ptr(), d_buf.data_ptr(), d_ok.data_ptr() + 4,
                d_hits.data_ptr(), 4, d_n.data_ptr(), d_ws.data_ptr(), 1 << 20, st, index_base=BASE, d_n_candidates=d_n.data_ptr() + 8),
            lambda: bv.prove_serialized_outputs_device(d_buf.data_ptr(), d_buf.data_ptr(), outs, d_ok.data_ptr() + 4, d_hits.data_ptr(),
                                                       d_ws.data_ptr(), 1 << 20, st, transcript=True),
        )
        for call in calls:
            with pytest.raises(B.BppError) as ei:
                call()
            assert ei.value.code == -1 and "outs_of[4] = %d" % bad in str(ei.value)
        torch.cuda.synchronize()
        assert (d_ok.cpu().numpy().view(np.uint32) == GUARD).all() and (d_hits.cpu().numpy().view(np.uint32) == GUARD).all()
        assert (d_n.cpu().numpy().view(np.uint32) == GUARD).all() and (d_ws.cpu().numpy() == 0x5a).all()
        # the host twins name it too
        with pytest.raises(B.BppError) as ei:
            bv.verify_serialized_outputs(blk["raw"], blk["cm"], outs, transcript=True)
        assert "outs_of[4] = %d" % bad in str(ei.value)
        with pytest.raises(B.BppError) as ei:
            bv.prove_serialized_outputs([[1] * o for o in outs], [[1] * o for o in outs])
        assert "outs_of[4] = %d" % bad in str(ei.value)
