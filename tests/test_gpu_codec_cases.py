"""-m gpu: the point codecs (csrc/codec.hpp, csrc/ristretto.hpp) and the generator hashing (csrc/hash_to_group.hpp) on the
device against the restatement (oracle/pyref.py), bit for bit, on the corpora of tests/codec_cases.py.

What makes "equal on the corpus" a statement about branches is the census of tests/test_codec_cases_cpu.py: the corpora
reach all 32 branch combinations of rist_decode and of rist_encode, every rejection reason, x at the modulus and at every
30-bit limb and 32-bit word boundary with both flags, y on both sides of (p - 1) / 2 and one step of every word away from
it, try-and-increment counters past 0, both parity outcomes and all 8 traces of the ristretto MAP in the hashed keys.
Every assertion compares with pyref; the device-pointer entry is first compared with pyref and then with the host-pointer
entry.  The inputs of the element derivation that no ABI call can deliver (t >= p) are pinned by the host build of the
same header (tests/host/ristretto_host_test.cpp)."""

import functools
import itertools

import numpy as np
import pytest

import codec_cases as CC
import oracle as O
import pyref as P
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

R = P.Ristretto255
CURVE_NAMES = ["bls12_381", "secp256k1", "ed25519"]
GUARD = 0x77


def _raw(datas):
    return np.frombuffer(b"".join(datas), dtype=np.uint8).reshape(len(datas), -1).copy()


def _arith(cname):
    need_gpu()
    import bulletproofsplus_amd as B
    return B, B.Arith.init(cname)


def _group(cname):
    return CC._edwards() if cname == "ed25519" else P.WeierstrassGroup(P.CURVES[cname])


def _check_decoded(cname, datas, want, pts, ok, what=""):
    """the device's answer for `datas` against want = [(verdict, point)]: verdict word, exact coordinates, and the wire's
    infinity where the string is turned down"""
    cid = O.CURVE_IDS[cname]
    inf = O.point_to_wire(cid, None)
    assert ok.tolist() == [0 if v else 1 for v, _ in want], \
        what + str([(i, datas[i].hex()) for i in range(len(datas)) if int(ok[i]) != (0 if want[i][0] else 1)][:6])
    for i, (v, q) in enumerate(want):
        if not v or q is None:
            assert np.array_equal(pts[i], inf), (what, i, datas[i].hex())
        elif q == (0, 1) and cname == "ed25519":
            assert O.wire_to_point(cid, pts[i]) in (None, (0, 1)), (what, i)   # the identity: either wire form
        else:
            assert np.array_equal(pts[i], O.point_to_wire(cid, q)), (what, i, datas[i].hex())


def _decode_corpus(cname):
    """-> (strings, [(verdict, point)]) of the plain codec, in corpus order"""
    if cname == "ed25519":
        cases = CC.rist_decode_cases()
        return [c.data for c in cases], [(c.point is not None, c.point) for c in cases]
    cases = CC.weierstrass_decode_cases(cname)
    datas, want = [c.data for c in cases], [(c.ok, c.point) for c in cases]
    if cname == "bls12_381":
        datas += [c.data for c in CC.bls_half_cases()]
        want += [(True, c.point) for c in CC.bls_half_cases()]
    return datas, want


@functools.lru_cache(maxsize=None)
def _encode_corpus(cname):
    """-> (points, encodings by pyref): ristretto255 the encode corpus; Weierstrass the accepted points of the sweep and of
    the flag cases (infinity among them), the bls_half points, and 1 g .. 64 g"""
    curve = P.CURVES[cname]
    if cname == "ed25519":
        cases = CC.rist_encode_cases()
        return [c.point for c in cases], [c.data for c in cases]
    pts = [c.point for c in CC.weierstrass_decode_cases(cname) if c.ok]
    if cname == "bls12_381":
        pts += [c.point for c in CC.bls_half_cases()]
    G = _group(cname)
    acc = None
    for _ in range(64):
        acc = G.add(acc, G.base())
        pts.append(acc)
    return pts, [P.compress_point(curve, q) for q in pts]


# ---- ristretto255 --------------------------------------------------------------------------------------------------------
def test_ristretto255_decode_corpus():
    B, a = _arith("ed25519")
    datas, want = _decode_corpus("ed25519")
    assert all(P.decompress_point(P.ED25519, d) == w for d, w in zip(datas[::7], want[::7]))
    pts, ok = B.decompress_points(a, _raw(datas))
    _check_decoded("ed25519", datas, want, pts, ok)
    assert 100 < int(ok.sum()) < len(datas) - 100


def test_ristretto255_encode_corpus():
    B, a = _arith("ed25519")
    cases = CC.rist_encode_cases()
    pts, want = _encode_corpus("ed25519")
    enc = B.compress_points(a, O.points_to_wire(O.ED25519, pts))
    bad = [(c.note, c.trace) for c, row in zip(cases, enc) if bytes(row) != R.encode(c.point)]
    assert not bad, bad[:6]
    # the four representatives of a coset give the same bytes (and the identity also as the wire's infinity)
    for _, grp in itertools.groupby(zip(cases, enc), key=lambda t: t[0].coset):
        assert len({bytes(row) for _, row in grp}) == 1
    assert bytes(B.compress_points(a, O.points_to_wire(O.ED25519, [None]))[0]) == R.encode(None) == bytes(32)
    # decode o encode: the restatement's representative of the coset
    back, ok = B.decompress_points(a, enc)
    _check_decoded("ed25519", want, [(True, R.decode(d)) for d in want], back, ok)


# ---- short Weierstrass -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", ["bls12_381", "secp256k1"])
def test_weierstrass_decode_corpus(cname):
    B, a = _arith(cname)
    curve = P.CURVES[cname]
    datas, want = _decode_corpus(cname)
    assert all(P.decompress_point(curve, d) == ((True, q) if v else (False, None)) for d, (v, q) in zip(datas, want))
    pts, ok = B.decompress_points(a, _raw(datas))
    _check_decoded(cname, datas, want, pts, ok)
    assert 50 < int(ok.sum()) < len(datas) - 50


@pytest.mark.parametrize("cname", ["bls12_381", "secp256k1"])
def test_weierstrass_compress_corpus(cname):
    B, a = _arith(cname)
    cid = O.CURVE_IDS[cname]
    pts, want = _encode_corpus(cname)
    enc = B.compress_points(a, O.points_to_wire(cid, pts))
    bad = [(i, pts[i]) for i in range(len(pts)) if bytes(enc[i]) != want[i]]
    assert not bad, bad[:4]
    if cname == "bls12_381":
        half = CC.bls_half_cases()
        henc = B.compress_points(a, O.points_to_wire(cid, [c.point for c in half]))
        for c, row in zip(half, henc):
            assert bytes(row) == c.data and bool(row[0] & 0x20) == c.above, c.note
        for pos, neg in zip(henc[0::2], henc[1::2]):
            assert pos[0] ^ neg[0] == 0x20 and bytes(pos[1:]) == bytes(neg[1:])


# ---- the device entry: launch geometry and guard words -----------------------------------------------------------------------
def _decompress_device(torch, a, raw, n, check_subgroup):
    """bpp_points_decompress_device on the first n strings of raw, into buffers one element longer than n and pre-filled
    -> (points (n + 1, PW) u64, ok (n + 1,) u32)"""
    from bulletproofsplus_amd import _lib
    dev = torch.device("cuda:0")
    fill64 = int.from_bytes(bytes([GUARD]) * 8, "little")
    d_in = torch.from_numpy(np.ascontiguousarray(raw[:n])).to(dev)
    d_pts = torch.full((n + 1, a.PW), fill64, dtype=torch.int64, device=dev)
    d_ok = torch.full((n + 1,), fill64 & 0xFFFFFFFF, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().bpp_points_decompress_device(a.handle, d_in.data_ptr(), n, d_pts.data_ptr(), d_ok.data_ptr(),
                                                       check_subgroup, torch.cuda.current_stream().cuda_stream),
               "bpp_points_decompress_device")
    torch.cuda.synchronize()
    return d_pts.cpu().numpy().view(np.uint64), d_ok.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def _subgroup_corpus():
    """BLS12-381 strings for check_subgroup = 1 with the verdict of the DEFINITION ([r] P = O): 4 points of G1, the order-3
    point (0, 2), the bls_half points, then the front of the decode corpus"""
    curve = P.BLS12_381
    G = _group("bls12_381")
    g1 = [G.mul(G.base(), k) for k in (1, 2, curve["r"] - 1, 0xC0DEC0DEC0DEC0DE)]
    datas = [P.compress_point(curve, q) for q in g1 + [(0, 2)]] + [c.data for c in CC.bls_half_cases()]
    datas += [c.data for c in CC.weierstrass_decode_cases("bls12_381")]
    datas = datas[:129]
    want = []
    for d in datas:
        v, q = P.decompress_point(curve, d)
        v = bool(v) and P.point_in_prime_subgroup(curve, G, q)
        want.append((v, q if v else None))
    assert [v for v, _ in want[:5]] == [True] * 4 + [False] and not any(v for v, _ in want[5:5 + 98])
    return datas, want


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_device_entry_geometry_and_guards(cname):
    """k_points_decompress has 64-lane blocks: n at 1, either side of one block and past two, through the entry the
    serialized path is built on; nothing is written past n"""
    torch = need_gpu()
    B, a = _arith(cname)
    datas, want = _decode_corpus(cname)
    raw = _raw(datas)
    host_pts, host_ok = B.decompress_points(a, raw[:129])
    _check_decoded(cname, datas[:129], want[:129], host_pts, host_ok, "host-pointer entry ")
    sub_datas, sub_want = _subgroup_corpus() if cname == "bls12_381" else (datas, want)
    sub_raw = _raw(sub_datas)
    for n in (1, 63, 64, 65, 129):
        pts, ok = _decompress_device(torch, a, raw, n, 0)
        _check_decoded(cname, datas[:n], want[:n], pts[:n], ok[:n], "n = %d " % n)
        assert np.array_equal(pts[:n], host_pts[:n]) and np.array_equal(ok[:n], host_ok[:n])
        assert (pts[n:].view(np.uint8) == GUARD).all() and (ok[n:].view(np.uint8) == GUARD).all(), n
        pts, ok = _decompress_device(torch, a, sub_raw, n, 1)
        _check_decoded(cname, sub_datas[:n], sub_want[:n], pts[:n], ok[:n], "check_subgroup, n = %d " % n)
        assert (pts[n:].view(np.uint8) == GUARD).all() and (ok[n:].view(np.uint8) == GUARD).all(), n
    if cname == "bls12_381":
        assert [int(v) for v in ok[:5]] == [0, 0, 0, 0, 1] and 0 < int(ok[:129].sum()) < 129


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_compress_geometry(cname):
    """k_points_compress has 128-lane blocks: n at 1, either side of one block and past it"""
    B, a = _arith(cname)
    pts, want = _encode_corpus(cname)
    wire = O.points_to_wire(O.CURVE_IDS[cname], pts)
    assert len(pts) >= 129
    for n in (1, 127, 128, 129):
        enc = B.compress_points(a, wire[:n])
        assert enc.shape == (n, B.compressed_bytes(a)) and [bytes(r) for r in enc] == want[:n], n


# ---- through the container decoder --------------------------------------------------------------------------------------------
def test_ristretto255_strings_through_the_container_decoder():
    """decode-corpus strings in the A slot of a valid (4, 2) proof: status 2 exactly where the restatement turns the string
    down, and the untouched proofs between them stay 0"""
    B, a = _arith("ed25519")
    c = P.ED25519
    G = _group("ed25519")
    n, m = 4, 2
    pk = P.PublicKey(G, n * m)
    prover = P.RangeProver()
    for v, gm in ((9, 5), (3, 6)):
        prover.commit(pk, v, gm)
    blob = P.encode_proof(c, n, m, P.RangeProof.prove(pk, n, prover))
    assert len(blob) == B.proof_bytes(a, n, m) and P.decode_proof(c, G, n, m, blob) is not None
    cases = CC.rist_decode_cases()
    picked = [x for x in cases if x.note != "random"]
    picked += [x for x in cases if x.note == "random" and x.point is None][:48 - len(picked)]
    assert len(picked) == 48 and {x.reason for x in picked} >= set(CC.REASONS)
    picked += [x for x in cases if x.note == "random" and x.point is not None][:8]
    blobs = np.stack([np.frombuffer(blob, dtype=np.uint8)] * (2 * len(picked) + 1))
    for i, x in enumerate(picked):
        blobs[2 * i + 1, 12:44] = np.frombuffer(x.data, dtype=np.uint8)
    want = [0 if P.decode_proof(c, G, n, m, bytes(row)) is not None else 2 for row in blobs]
    assert want[0::2] == [0] * (len(picked) + 1) and want[1::2] == [0 if x.point is not None else 2 for x in picked]
    assert want.count(0) - len(picked) - 1 >= 8
    _, _, st = B.decode_proofs(a, n, m, blobs)
    assert st.tolist() == want


# ---- hashed generators ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_hashed_keys_equal_the_restatement(cname):
    """81 generators are two blocks of k_hash_to_group, the second ragged; the labels cross every SHA-256 padding boundary
    of the seed's message; a shorter key is a prefix of a longer one (csrc/mixed.hpp relies on it)"""
    B, a = _arith(cname)
    cid = O.CURVE_IDS[cname]
    G = _group(cname)
    keys = {}
    for label, length, pts in CC.hashed_key_cases(cname):
        pk = B.PublicKey.hashed(a, length, label)
        keys[(label, length)] = pk
        assert pk.G_vec.shape == pk.H_vec.shape == (length, a.PW)
        assert O.wire_to_point(cid, pk.gh[0]) == G.base()
        got = np.concatenate([pk.gh[1:], pk.G_vec, pk.H_vec])
        want = O.points_to_wire(cid, [hp.point for hp in pts])
        bad = [(i, pts[i].ctr, pts[i].flipped, pts[i].maps) for i in range(len(pts)) if not np.array_equal(got[i], want[i])]
        assert not bad, (label, length, bad[:6])
    long, short = keys[(CC.LABEL, 40)], keys[(CC.LABEL, 8)]
    want_long = O.points_to_wire(cid, [hp.point for hp in CC.hashed_key_cases(cname)[0][2]])
    assert np.array_equal(short.gh, np.concatenate([O.points_to_wire(cid, [G.base()]), want_long[:1]]))
    assert np.array_equal(short.G_vec, want_long[1:9]) and np.array_equal(short.H_vec, want_long[41:49])
    first = [bytes(pk.gh[1]) + bytes(pk.G_vec[0]) + bytes(pk.H_vec[0]) for (lb, ln), pk in keys.items() if ln != 8]
    assert len(first) == 8 and len(set(first)) == 8                       # label-separated
    hs = [bytes(pk.gh[1]) for (lb, ln), pk in keys.items() if ln != 8]
    assert len(set(hs)) == 8
