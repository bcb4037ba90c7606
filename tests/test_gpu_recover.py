"""-m gpu: mask recovery and scanning (bpp_range_recover_masks_mixed*, bpp_range_scan_serialized_mixed*; csrc/recover.hpp).

The expected Gamma_i = gamma_0 + z^2 gamma_1 + .. always comes from the gammas the test chose and from a z the CHECKER drew
(the C oracle's verifier with want_challenges, pyref's FsTranscript on edwards25519; the reference's literals in literal
mode) -- recover_cases.gamma_of -- never from the library.  Proofs are the oracle's (BLS12-381, secp256k1), pyref's with its
blinding attributes set (edwards25519) or, where the test is about lane groups and the scan, the device prover's."""

import functools
import hashlib
import random

import numpy as np
import pytest

import oracle as O
import pyref as P
import recover_cases as RC
import verdict_corpus as VC
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

CID = {"bls12_381": 0, "secp256k1": 1, "ed25519": 2}
CURVES = ("bls12_381", "secp256k1", "ed25519")
N, CAP, WB = 8, 4, 5
KEY = hashlib.sha256(b"recover blinding key").digest()
KEY2 = hashlib.sha256(b"another blinding key").digest()
BASE = (1 << 33) + 5
MS = [1, 2, 1, 4, 1]


def _k(n, m):
    return (n * m).bit_length() - 1


@functools.lru_cache(maxsize=None)
def _corpus(cname, n, m):
    return VC.Corpus(cname, n, m, False)


def _engine(cname, n=N, cap=CAP, wb=WB):
    import bulletproofsplus_amd as B
    cp = _corpus(cname, n, cap)
    a = B.Arith(cname)
    return B, a, B.BatchVerifier(B.PublicKey.from_points(a, cp.gh, cp.G, cp.H), n, cap, window_bits=wb)


def _dev(torch, x):
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.uint8).reshape(-1)).to(torch.device("cuda:0"))


def _inputs(cname, ms, n, seed):
    r = RC.ORDER[cname]
    rng = random.Random(seed)
    vals = [[rng.randrange(1 << min(n, 31)) for _ in range(m)] for m in ms]
    gams = [[rng.randrange(1, r) for _ in range(m)] for m in ms]
    gams[0][0] = r - 1
    return vals, gams


def _pyref_proof(cname, n, values, gammas, blind7):
    """edwards25519: pyref under the transcript with its blinding attributes set -- pyref has one d_L, d_R for all rounds.
    blind7 = [alpha, r, s, delta, eta, d_L, d_R] -> (record, triple ints, challenge ints, the 5 + 2k blinding scalars)"""
    m = len(values)
    cp = _corpus(cname, n, m)
    k = _k(n, m)
    T = P.Transcript
    saved = (T.ALPHA_SINGLE, T.ALPHA_MULTI, T.R, T.S, T.DELTA, T.ETA, T.D_L, T.D_R)
    fs = P.FsTranscript(cp.curve, CID[cname], n, m, cp.ppk)
    T.ALPHA_SINGLE = T.ALPHA_MULTI = blind7[0]
    T.R, T.S, T.DELTA, T.ETA, T.D_L, T.D_R = blind7[1:]
    T.fs = fs
    try:
        pts, sc, V = cp.prove(values, gammas)
    finally:
        T.fs = None
        (T.ALPHA_SINGLE, T.ALPHA_MULTI, T.R, T.S, T.DELTA, T.ETA, T.D_L, T.D_R) = saved
    ch = _pyref_challenges(cname, n, m, np.concatenate([pts, V]), sc)
    return np.concatenate([pts, V]), [int(x) for x in O.wire_to_scalars(sc)], ch, blind7[:5] + [blind7[5]] * k + [blind7[6]] * k


def _pyref_challenges(cname, n, m, rec, sc):
    """[y, z, e, e_1..e_k] of a wire record by pyref's restatement of the transcript"""
    cp = _corpus(cname, n, m)
    k = _k(n, m)
    fs = P.FsTranscript(cp.curve, CID[cname], n, m, cp.ppk)
    pp = O.wire_to_points(CID[cname], rec)
    red = [int(x) for x in O.wire_to_scalars(sc)]
    pf = P.RangeProof(pp[0], P.WeightedInnerProductProof(pp[3:3 + k], pp[3 + k:3 + 2 * k], pp[1], pp[2], *red))
    ch = fs.verifier_challenges(pf, pp[3 + 2 * k:])
    return [ch["y"], ch["z"], ch["e"]] + list(ch["e_rounds"])


def _checker_challenges(cname, n, m, rec, sc):
    """the challenge block of a record made elsewhere, drawn by the checker"""
    if cname == "ed25519":
        return _pyref_challenges(cname, n, m, rec, sc)
    k = _k(n, m)
    O.set_transcript(True)
    try:
        rc, _, _, ch = O.range_verify(O.PublicKey(CID[cname], n * m), n, m, rec[:3 + 2 * k], sc, rec[3 + 2 * k:],
                                      want_challenges=True)
    finally:
        O.set_transcript(False)
    return [int(x) for x in O.wire_to_scalars(ch)]


@functools.lru_cache(maxsize=None)
def _made(cname):
    """MS proofs at index BASE + i under KEY, by the checker's prover -> [(record, triple, ch, blind, gammas)]"""
    r = RC.ORDER[cname]
    vals, gams = _inputs(cname, MS, N, 5100 + CID[cname])
    out = []
    for i, m in enumerate(MS):
        k = _k(N, m)
        if cname == "ed25519":
            full = O.blinding_from_key(KEY, BASE + i, k, r)
            rec, triple, ch, blind = _pyref_proof(cname, N, vals[i], gams[i], full[:5] + [full[5], full[5 + k]])
        else:
            p = RC.oracle_proof(cname, N, vals[i], gams[i], True, O.blinding_from_key(KEY, BASE + i, k, r))
            rec, triple, ch, blind = RC.record(p), p["triple"], p["ch"], p["blind"]
        out.append((rec, triple, ch, blind, gams[i]))
    return out


def _recover_device(torch, bv, ms, triples, d_ch=None, **kw):
    """-> [Gamma_i] through bpp_range_recover_masks_mixed_device; kw: blind_key, index_base, index (ints), blinding (ints).
    d_out_masks sits between two guards of 64 bytes, which must come back as they went in."""
    count = len(ms)
    guard = 64
    d_sc = _dev(torch, O.scalars_to_wire([x for t in triples for x in t]))
    d_all = torch.full((count * 32 + 2 * guard,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_out = d_all[guard:guard + count * 32]
    wsb = bv.recover_workspace_bytes(ms)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    d_ix = _dev(torch, np.array(kw["index"], dtype=np.uint64)) if kw.get("index") is not None else None
    d_bl = _dev(torch, O.scalars_to_wire([x for b in kw["blinding"] for x in b])) if kw.get("blinding") is not None else None
    bv.recover_masks_device(d_sc.data_ptr(), ms, d_out.data_ptr(), d_ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream,
                            d_challenges=d_ch.data_ptr() if d_ch is not None else 0, blind_key=kw.get("blind_key"),
                            index_base=kw.get("index_base", 0), d_index=d_ix.data_ptr() if d_ix is not None else 0,
                            d_blinding=d_bl.data_ptr() if d_bl is not None else 0)
    torch.cuda.synchronize()
    got = d_all.cpu().numpy()
    assert (got[:guard] == 0x5a).all() and (got[guard + count * 32:] == 0x5a).all(), "a store outside d_out_masks"
    return [int(x) for x in O.wire_to_scalars(got[guard:guard + count * 32].copy().view(np.uint64).reshape(count, 4))]


def _derive(torch, bv, ms, recs):
    """bpp_verifier_derive_challenges_mixed on the packed records -> (device buffer, [[ints]] per proof)"""
    d_p = _dev(torch, np.concatenate(recs))
    nch = [3 + _k(bv.n, m) for m in ms]
    d_ch = torch.zeros((sum(nch) * 32,), dtype=torch.uint8, device="cuda:0")
    wsb = bv.mixed_workspace_bytes(ms)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    bv.derive_challenges_mixed_device(d_p.data_ptr(), ms, d_ch.data_ptr(), d_ws.data_ptr(), wsb,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flat = [int(x) for x in O.wire_to_scalars(d_ch.cpu().numpy().view(np.uint64).reshape(-1, 4))]
    off = np.concatenate([[0], np.cumsum(nch)]).astype(int)
    return d_ch, [flat[off[i]:off[i + 1]] for i in range(len(ms))]


@pytest.mark.parametrize("cname", CURVES)
def test_wire_call_recovers_checker_made_proofs(cname):
    """ms = [1, 2, 1, 4, 1] at index_base 2^33 + 5, transcript and key-derived blinding: derive_challenges_mixed, then the
    recover call; Gamma_i exact.  The same for the proofs shuffled with d_index, and for d_blinding.  edwards25519: pyref's
    proofs (one d_L, d_R for all rounds) with the same scalars passed as d_blinding."""
    torch = need_gpu()
    r = RC.ORDER[cname]
    made = _made(cname)
    B, a, bv = _engine(cname)
    recs, triples = [x[0] for x in made], [x[1] for x in made]
    want = [RC.gamma_of(r, g, ch[1]) for _, _, ch, _, g in made]
    for (rec, triple, ch, blind, g), w, m in zip(made, want, MS):   # the checker's own algebra closes
        assert RC.recover_bigint(r, N, m, triple[2], ch, blind) == w
    d_ch, got_ch = _derive(torch, bv, MS, recs)
    assert got_ch == [x[2] for x in made]
    blinds = [x[3] for x in made]
    assert _recover_device(torch, bv, MS, triples, d_ch, blinding=blinds) == want
    if cname != "ed25519":
        assert _recover_device(torch, bv, MS, triples, d_ch, blind_key=KEY, index_base=BASE) == want
        # the host twin behind the Python wrapper, challenges as the per-proof blocks
        blocks = [O.scalars_to_wire(c) for c in got_ch]
        assert bv.recover_masks(O.scalars_to_wire([x for t in triples for x in t]).reshape(-1, 3, 4), MS, blocks, blind_key=KEY,
                                index_base=BASE) == want
        # a wrong key, an index base off by one: other numbers
        for kw in (dict(blind_key=KEY2, index_base=BASE), dict(blind_key=KEY, index_base=BASE + 1)):
            got = _recover_device(torch, bv, MS, triples, d_ch, **kw)
            assert all(x != w for x, w in zip(got, want))
    # a scanner does not see proofs in the order they were made
    perm = [3, 0, 4, 1, 2]
    ms_p = [MS[j] for j in perm]
    d_chp, _ = _derive(torch, bv, ms_p, [recs[j] for j in perm])
    kw = dict(blinding=[blinds[j] for j in perm]) if cname == "ed25519" else dict(blind_key=KEY, index=[BASE + j for j in perm])
    assert _recover_device(torch, bv, ms_p, [triples[j] for j in perm], d_chp, **kw) == [want[j] for j in perm]
    if cname != "ed25519":
        assert bv.recover_masks(O.scalars_to_wire([x for j in perm for x in triples[j]]).reshape(-1, 3, 4), ms_p,
                                [O.scalars_to_wire(got_ch[j]) for j in perm], blind_key=KEY,
                                index=[BASE + j for j in perm]) == [want[j] for j in perm]
    bv.close()


@pytest.fixture(scope="module")
def engine_64_16():
    """a (64, 16) BLS12-381 engine at window_bits 5: the capacity shape, k = 10"""
    need_gpu()
    import bulletproofsplus_amd as B
    a = B.Arith("bls12_381")
    bv = B.BatchVerifier(B.PublicKey.new(a, 64 * 16), 64, 16, window_bits=WB)
    yield B, a, bv
    bv.close()


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_literal_mode(cname):
    """both sources NULL, d_challenges NULL: Gamma from reference-parity proofs of (8, 1) and (8, 4)"""
    torch = need_gpu()
    r = RC.ORDER[cname]
    ms = [1, 4, 4, 1]
    vals, gams = _inputs(cname, ms, N, 5200 + CID[cname])
    proofs = [RC.oracle_proof(cname, N, v, g, False) for v, g in zip(vals, gams)]
    want = [RC.gamma_of(r, g, p["ch"][1]) for p, g in zip(proofs, gams)]
    assert want[0] == gams[0][0] and want[3] == gams[3][0]
    B, a, bv = _engine(cname)
    assert _recover_device(torch, bv, ms, [p["triple"] for p in proofs]) == want
    assert bv.recover_masks(np.stack([p["scalars"] for p in proofs]), ms) == want
    bv.close()


def test_literal_mode_golden_64_16(golden, engine_64_16):
    """Literal mode from the golden (64, 16) proof's scalars, beside the golden (64, 2) proof, on a (64, 16) engine"""
    torch = need_gpu()
    B, a, bv = engine_64_16
    r = RC.ORDER["bls12_381"]
    cases = [golden("protocol_full_bls12_381.json")[i] for i in (2, 0)]
    assert [(c["n"], c["m"]) for c in cases] == [(64, 16), (64, 2)]
    triples = [[int(c[f], 16) for f in ("r_prime", "s_prime", "d_prime")] for c in cases]
    want = [RC.gamma_of(r, [int(g) for g in c["gammas"]], 23) for c in cases]   # z = 23: range/mod.rs:279
    assert _recover_device(torch, bv, [16, 2], triples) == want


def _prove_device(torch, bv, vals, gams, key, base, amount64=False):
    """the device prover under the transcript with a blind key -> (records, triples as ints)"""
    ms = [len(v) for v in vals]
    PW, n = bv.arith.PW, bv.n
    v = np.array([int(x) for row in vals for x in row], dtype=np.uint64)
    g = O.scalars_to_wire([int(x) for row in gams for x in row])
    d_v, d_g = _dev(torch, v), _dev(torch, g)
    nv = [3 + 2 * _k(n, m) + m for m in ms]
    d_p = torch.zeros((sum(nv) * PW * 8,), dtype=torch.uint8, device="cuda:0")
    d_s = torch.zeros((len(ms) * 96,), dtype=torch.uint8, device="cuda:0")
    wsb = bv.prover_mixed_workspace_bytes(ms)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    bv.prove_mixed_device(d_v.data_ptr(), d_g.data_ptr(), ms, d_p.data_ptr(), d_s.data_ptr(), d_ws.data_ptr(), wsb,
                          torch.cuda.current_stream().cuda_stream, transcript=True, blind_key=key, index_base=base,
                          amount64=amount64)
    torch.cuda.synchronize()
    pts = d_p.cpu().numpy().view(np.uint64).reshape(-1, PW)
    off = np.concatenate([[0], np.cumsum(nv)]).astype(int)
    sc = d_s.cpu().numpy().view(np.uint64).reshape(len(ms), 3, 4)
    return [pts[off[i]:off[i + 1]] for i in range(len(ms))], sc


@pytest.mark.parametrize("count", (1, 5, 67))
def test_lane_groups_short_last_wave(count):
    """(8, 1) proofs by the device prover under the transcript with a blind key: four proofs per wave, a short last wave;
    for a single output Gamma is the mask itself, whatever z"""
    torch = need_gpu()
    cname = "secp256k1"
    r = RC.ORDER[cname]
    B, a, bv = _engine(cname, N, 1)
    rng = random.Random(5300 + count)
    vals = [[rng.randrange(256)] for _ in range(count)]
    gams = [[rng.randrange(r)] for _ in range(count)]
    recs, sc = _prove_device(torch, bv, vals, gams, KEY, BASE)
    ms = [1] * count
    d_ch, _ = _derive(torch, bv, ms, recs)
    triples = [[int(x) for x in O.wire_to_scalars(sc[i])] for i in range(count)]
    assert _recover_device(torch, bv, ms, triples, d_ch, blind_key=KEY, index_base=BASE) == [g[0] for g in gams]
    bv.close()


def test_lane_groups_largest_term_count(engine_64_16):
    """one call with two proofs at the capacity (64, 16) and one (64, 1): k = 10 and k = 6, twelve and eight of a group's
    sixteen lanes; z from the oracle's verifier"""
    torch = need_gpu()
    cname = "bls12_381"
    r = RC.ORDER[cname]
    B, a, bv = engine_64_16
    ms = [16, 1, 16]
    vals, gams = _inputs(cname, ms, 64, 5400)
    recs, sc = _prove_device(torch, bv, vals, gams, KEY, BASE)
    zs = [_checker_challenges(cname, 64, m, recs[i], sc[i])[1] for i, m in enumerate(ms)]
    want = [RC.gamma_of(r, g, z) for g, z in zip(gams, zs)]
    assert want[1] == gams[1][0]
    d_ch, _ = _derive(torch, bv, ms, recs)
    triples = [[int(x) for x in O.wire_to_scalars(sc[i])] for i in range(len(ms))]
    assert _recover_device(torch, bv, ms, triples, d_ch, blind_key=KEY, index_base=BASE) == want


# ---- scan from bytes ---------------------------------------------------------------------------------------------------
SCAN_MS = [1, 1, 1, 1, 2, 4, 1]
OWN, OTHER, WRONG, DAMAGED, BIG = 0, 1, 2, 3, 6
BIG_AMOUNT = (1 << 31) + 5


def _split_bytes(B, a, raw, cm, ms, version):
    pb = B.uncompressed_bytes(a) if version == 2 else B.compressed_bytes(a)
    po = np.concatenate([[0], np.cumsum([B.proof_bytes(a, N, m, version) for m in ms])]).astype(int)
    co = np.concatenate([[0], np.cumsum([m * pb for m in ms])]).astype(int)
    return [raw[po[i]:po[i + 1]] for i in range(len(ms))], [cm[co[i]:co[i + 1]] for i in range(len(ms))]


def _scan_block(cname, amount64, version):
    """-> (bv, proofs bytes, commitment bytes, amounts, want status, want masks): a block made by the device prover under KEY
    at BASE + i; container OTHER is the same output proved under KEY2, WRONG gets another candidate amount, DAMAGED a flipped
    header byte, BIG an amount of 2^31 + 5"""
    r = RC.ORDER[cname]
    B, a, bv = _engine(cname)
    vals, gams = _inputs(cname, SCAN_MS, N, 5500 + CID[cname])
    vals[BIG] = [BIG_AMOUNT]
    unc = version == 2
    kw = dict(transcript=True, index_base=BASE, uncompressed=unc, amount64=amount64)
    raw, cm, ms = bv.prove_serialized_mixed(vals, gams, blind_key=KEY, **kw)
    raw2, cm2, _ = bv.prove_serialized_mixed(vals, gams, blind_key=KEY2, **kw)
    assert ms.tolist() == SCAN_MS and len(raw) == len(raw2) and cm == cm2
    pr, cs = _split_bytes(B, a, raw, cm, SCAN_MS, version)
    pr2, _ = _split_bytes(B, a, raw2, cm2, SCAN_MS, version)
    assert pr[OTHER] != pr2[OTHER]
    pr[OTHER] = pr2[OTHER]
    bad = bytearray(pr[DAMAGED])
    bad[7] ^= 3   # the header's m
    pr[DAMAGED] = bytes(bad)
    amounts = [v[0] for v in vals]
    amounts[WRONG] += 1
    # Gamma of the aggregated proofs: z by the checker, on the wire records of the same proofs (prove_batch_mixed)
    recs, sc = bv.prove_batch_mixed(vals, gams, transcript=True, blind_key=KEY, index_base=BASE, amount64=amount64)
    gamma = [RC.gamma_of(r, g, _checker_challenges(cname, N, m, recs[i], sc[i])[1] if m > 1 else 0)
             for i, (m, g) in enumerate(zip(SCAN_MS, gams))]
    status = [0, 1, 1, 2, 3, 3, 0]
    masks = [gamma[i] if s in (0, 3) else 0 for i, s in enumerate(status)]
    return B, bv, b"".join(pr), b"".join(cs), amounts, status, masks, gamma


@pytest.mark.parametrize("amount64", (False, True))
@pytest.mark.parametrize("cname", CURVES)
def test_scan_from_bytes(cname, amount64):
    """prove_serialized_mixed with transcript and blind key, with and without amount64 (an amount of 2^31 + 5 in the block:
    `v as i32` on both sides without the flag, the whole u64 with it); a proof made under another key, one wrong candidate
    amount, one damaged header, m_i = 2 and 4: the exact status vector, the chosen gammas under status 0, zero under 1 and 2,
    Gamma under 3"""
    need_gpu()
    B, bv, raw, cm, amounts, status, masks, gamma = _scan_block(cname, amount64, 1)
    kw = dict(transcript=True, amount64=amount64, blind_key=KEY)
    st, got = bv.scan_serialized_mixed(raw, cm, SCAN_MS, index_base=BASE, amounts=amounts, **kw)
    assert st.tolist() == status and got == masks
    # the flag belongs to the proofs: with the other setting the big amount does not open its commitment
    st2, got2 = bv.scan_serialized_mixed(raw, cm, SCAN_MS, index_base=BASE, amounts=amounts, transcript=True,
                                         amount64=not amount64, blind_key=KEY)
    assert st2.tolist() == status[:BIG] + [1] and got2 == masks[:BIG] + [0]
    # no amounts: nothing is confirmed, Gamma as computed; the index as a list
    st, got = bv.scan_serialized_mixed(raw, cm, SCAN_MS, index=[BASE + i for i in range(len(SCAN_MS))], **kw)
    assert st.tolist() == [3, 3, 3, 2, 3, 3, 3]
    assert [g for i, g in enumerate(got) if i not in (OTHER, DAMAGED)] == [g for i, g in enumerate(gamma) if i not in (OTHER, DAMAGED)]
    assert got[DAMAGED] == 0 and got[OTHER] not in (0, gamma[OTHER])
    # the same scan shuffled: statuses and masks follow their proofs
    perm = [5, 0, 6, 3, 1, 4, 2]
    pr, cs = _split_bytes(B, bv.arith, raw, cm, SCAN_MS, 1)
    st, got = bv.scan_serialized_mixed(b"".join(pr[j] for j in perm), b"".join(cs[j] for j in perm), [SCAN_MS[j] for j in perm],
                                       index=[BASE + j for j in perm], amounts=[amounts[j] for j in perm], **kw)
    assert st.tolist() == [status[j] for j in perm] and got == [masks[j] for j in perm]
    bv.close()


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_scan_literal_mode(cname):
    """no BPP_SER_TRANSCRIPT, no blinding source: the reference's literal challenges and blinding.  Containers encoded from the
    C oracle's reference-parity proofs of (8, 1), (8, 4), (8, 1), (8, 2); the second single output gets a wrong amount"""
    need_gpu()
    r = RC.ORDER[cname]
    ms = [1, 4, 1, 2]
    vals, gams = _inputs(cname, ms, N, 5600 + CID[cname])
    proofs = [RC.oracle_proof(cname, N, v, g, False) for v, g in zip(vals, gams)]
    B, a, bv = _engine(cname)
    raw = b"".join(B.encode_proofs(a, N, m, p["points"][None], p["scalars"][None]).tobytes() for m, p in zip(ms, proofs))
    cm = b"".join(B.compress_points(a, p["V"]).tobytes() for p in proofs)
    gamma = [RC.gamma_of(r, g, p["ch"][1]) for p, g in zip(proofs, gams)]
    assert gamma[0] == gams[0][0] and [p["ch"][1] for p in proofs] == [7, 23, 7, 23]
    st, got = bv.scan_serialized_mixed(raw, cm, ms, amounts=[vals[0][0], 0, vals[2][0] + 1, 0])
    assert st.tolist() == [0, 3, 1, 3] and got == [gamma[0], gamma[1], 0, gamma[3]]
    st, got = bv.scan_serialized_mixed(raw, cm)   # framed from the bytes, nothing to confirm
    assert st.tolist() == [3, 3, 3, 3] and got == gamma
    bv.close()


def test_scan_version_2_containers():
    need_gpu()
    B, bv, raw, cm, amounts, status, masks, gamma = _scan_block("secp256k1", True, 2)
    st, got = bv.scan_serialized_mixed(raw, cm, SCAN_MS, transcript=True, uncompressed=True, amount64=True, blind_key=KEY,
                                       index_base=BASE, amounts=amounts)
    assert st.tolist() == status and got == masks
    bv.close()


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_host_twins_at_one_proof_and_a_small_block_with_and_without_the_optional_inputs(cname):
    """bpp_range_recover_masks_mixed and bpp_range_scan_serialized_mixed on host pointers, at one proof and at a block of
    mixed m_i: once with every optional input absent (literal challenges and blinding; no index, no amounts) and once with
    them present (challenges, key and index list or a blinding buffer; amounts), against the checker's Gamma"""
    need_gpu()
    r = RC.ORDER[cname]
    B, a, bv = _engine(cname)
    # absent: the C oracle's reference-parity proofs
    ms = [1, 4, 2, 1]
    vals, gams = _inputs(cname, ms, N, 5900 + CID[cname])
    proofs = [RC.oracle_proof(cname, N, v, g, False) for v, g in zip(vals, gams)]
    gamma = [RC.gamma_of(r, g, p["ch"][1]) for p, g in zip(proofs, gams)]
    raw = [B.encode_proofs(a, N, m, p["points"][None], p["scalars"][None]).tobytes() for m, p in zip(ms, proofs)]
    cm = [B.compress_points(a, p["V"]).tobytes() for p in proofs]
    for sel in ([0], [1], [0, 1, 2, 3]):
        ms_s, want = [ms[i] for i in sel], [gamma[i] for i in sel]
        assert bv.recover_masks(np.stack([proofs[i]["scalars"] for i in sel]), ms_s) == want, sel
        st, got = bv.scan_serialized_mixed(b"".join(raw[i] for i in sel), b"".join(cm[i] for i in sel), ms_s)
        assert st.tolist() == [3] * len(sel) and got == want, sel
    # present, recovery: the transcript's challenges with the key and an index list, and with a blinding buffer
    made = _made(cname)
    want = [RC.gamma_of(r, g, ch[1]) for _, _, ch, _, g in made]
    for sel in ([0], [3], [3, 0, 4, 1, 2]):
        sc = O.scalars_to_wire([x for j in sel for x in made[j][1]]).reshape(-1, 3, 4)
        ms_s, blocks = [MS[j] for j in sel], [O.scalars_to_wire(made[j][2]) for j in sel]
        assert bv.recover_masks(sc, ms_s, blocks, blind_key=KEY, index=[BASE + j for j in sel]) == [want[j] for j in sel], sel
        assert bv.recover_masks(sc, ms_s, blocks, blinding=[made[j][3] for j in sel]) == [want[j] for j in sel], sel
    bv.close()
    # present, scan: transcript, key, index list and candidate amounts
    B, bv, raw, cm, amounts, status, masks, _ = _scan_block(cname, False, 1)
    pr, cs = _split_bytes(B, bv.arith, raw, cm, SCAN_MS, 1)
    for sel in ([OWN], [WRONG], [5, 0, 6, 3, 1, 4, 2]):
        st, got = bv.scan_serialized_mixed(b"".join(pr[j] for j in sel), b"".join(cs[j] for j in sel), [SCAN_MS[j] for j in sel],
                                           transcript=True, blind_key=KEY, index=[BASE + j for j in sel],
                                           amounts=[amounts[j] for j in sel])
        assert st.tolist() == [status[j] for j in sel] and got == [masks[j] for j in sel], sel
    bv.close()


def test_errors_that_need_an_engine():
    """an m_i above the engine's m (the text names i), a workspace smaller than the layout: BPP_E_ARG, nothing written"""
    torch = need_gpu()
    B, a, bv = _engine("secp256k1")
    assert bv.recover_workspace_bytes([1, 8]) == 0 and bv.recover_workspace_bytes([1, 8], serialized=True) == 0
    d = torch.full((4096,), 0x5a, dtype=torch.uint8, device="cuda:0")
    p = d.data_ptr()
    with pytest.raises(B.BppError) as ei:
        bv.recover_masks_device(p, [1, 2, 8], p, p, 4096, blind_key=KEY)
    assert ei.value.code == -1 and "m_of[2]" in str(ei.value)
    with pytest.raises(B.BppError) as ei:
        bv.scan_serialized_mixed_device(p, p, [8, 1], p, p, p, 4096, transcript=True, blind_key=KEY)
    assert ei.value.code == -1 and "m_of[0]" in str(ei.value)
    ms = [1, 2, 4, 1]
    for serialized in (False, True):
        wsb = bv.recover_workspace_bytes(ms, serialized=serialized)
        assert wsb > 0
        d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(B.BppError) as ei:
            if serialized:
                bv.scan_serialized_mixed_device(p, p, ms, p, p, d_ws.data_ptr(), wsb - 1, transcript=True, blind_key=KEY)
            else:
                bv.recover_masks_device(p, ms, p, d_ws.data_ptr(), wsb - 1, blind_key=KEY)
        assert ei.value.code == -1 and "workspace too small" in str(ei.value)
    torch.cuda.synchronize()
    assert d.cpu().tolist() == [0x5a] * 4096
    bv.close()
