"""-m gpu: verifying a block and listing the outputs of many view keys in one call
(bpp_range_verify_find_serialized_mixed_keys*, bpp_amounts_seal*; csrc/find.hpp).

Expected values never come from the library.  The pad of a sealed amount is hashlib's (find_cases.pad).  Who owns an
output, its amount and its mask are the ones the test chose when it made the proof.  The verdict of a container is the
CHECKER's on the wire record of the same proof (the C oracle's verifier under the transcript, pyref on edwards25519), 2 for
the container the test damaged.  The hit list is built from those three.  The blocks are the device prover's, as in
tests/test_gpu_recover_keys.py, whose block and helpers are reused by import."""

import hashlib
import random

import numpy as np
import pytest

import find_cases as FC
import oracle as O
import pyref as P
import recover_cases as RC
import test_gpu_recover as TR
import test_gpu_recover_keys as TK
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

CID, CURVES, N, BASE = TR.CID, TR.CURVES, TR.N, TR.BASE
KEY, KEY2, KEYS = TK.KEY, TK.KEY2, TK.KEYS
SCAN_MS, OWN, OTHER, WRONG, DAMAGED, BIG = TR.SCAN_MS, TR.OWN, TR.OTHER, TR.WRONG, TR.DAMAGED, TR.BIG
MS = SCAN_MS + [1]
TAMPERED = len(SCAN_MS)   # a single output of KEY whose r' was incremented after proving
MAKER = [KEY2 if i == OTHER else KEY for i in range(len(MS))]
GUARD = 0x5a5a5a5a


def _checker_verdict(cname, m, rec, sc):
    """the verdict of a wire record under the transcript, by the checker"""
    k = TR._k(N, m)
    cp = TR._corpus(cname, N, m)
    pts, V = rec[:3 + 2 * k], rec[3 + 2 * k:]
    if cname == "ed25519":
        P.Transcript.fs = P.FsTranscript(cp.curve, CID[cname], N, m, cp.ppk)
        try:
            return cp.verdict(pts, sc, V)
        finally:
            P.Transcript.fs = None
    O.set_transcript(True)
    try:
        return cp.verdict(pts, sc, V)
    finally:
        O.set_transcript(False)


_blocks = {}


def _block(cname, amount64, version):
    """test_gpu_recover_keys._block's seven containers and TAMPERED behind them -> dict(bv, B, raw, cm, pr, cs, amounts,
    verdict (8, the checker's), status (3 x 8, the plain scan's), hits [(key_no, position, amount, mask)], sealed (8))"""
    if (cname, amount64, version) in _blocks:
        return _blocks[(cname, amount64, version)]
    r = RC.ORDER[cname]
    blk7 = TK._block(cname, amount64, version)
    B, bv = blk7["B"], blk7["bv"]
    a = bv.arith
    # the wire records of the seven, as _block made them, for the checker
    vals, gams = TR._inputs(cname, SCAN_MS, N, 5500 + CID[cname])
    vals[BIG] = [TR.BIG_AMOUNT]
    wkw = dict(transcript=True, index_base=BASE, amount64=amount64)
    recs, sc = bv.prove_batch_mixed(vals, gams, blind_key=KEY, **wkw)
    recs2, sc2 = bv.prove_batch_mixed(vals, gams, blind_key=KEY2, **wkw)
    recs, sc = list(recs), [np.array(x) for x in sc]
    recs[OTHER], sc[OTHER] = recs2[OTHER], np.array(sc2[OTHER])
    # the eighth: made under KEY at its own index, then r' + 1
    tv, tg = [[173]], [[(7 * r) // 11]]
    tkw = dict(transcript=True, blind_key=KEY, index_base=BASE + TAMPERED, amount64=amount64)
    traw, tcm, _ = bv.prove_serialized_mixed(tv, tg, uncompressed=version == 2, **tkw)
    trec, tsc = bv.prove_batch_mixed(tv, tg, **tkw)
    traw = bytearray(bytes(traw))
    tail = len(traw) - 96   # the container ends with r', s', delta' as 32 little-endian bytes each
    rp = int.from_bytes(traw[tail:tail + 32], "little")
    assert rp == int(O.wire_to_scalars(tsc[0])[0])
    rp1 = (rp + 1) % r
    traw[tail:tail + 32] = rp1.to_bytes(32, "little")
    tsc1 = np.array(tsc[0])
    tsc1[0] = O.scalars_to_wire([rp1])[0]
    recs.append(trec[0])
    sc.append(tsc1)
    amounts = blk7["amounts"] + [tv[0][0]]
    verdict = [2 if i == DAMAGED else _checker_verdict(cname, m, recs[i], sc[i]) for i, m in enumerate(MS)]
    assert verdict[OWN] == verdict[OTHER] == verdict[WRONG] == 0 and verdict[TAMPERED] == 1 and verdict[4] == verdict[5] == 0
    # the plain scan answers for TAMPERED what it answers for OWN: the owner's key opens it
    status = [row + [0 if j == 0 else 1] for j, row in enumerate(blk7["status"])]
    masks = [row + [tg[0][0] if j == 0 else 0] for j, row in enumerate(blk7["masks"])]
    hits = [(j, i, amounts[i], masks[j][i]) for j in range(len(KEYS)) for i in range(len(MS))
            if MS[i] == 1 and verdict[i] == 0 and MAKER[i] == KEYS[j] and i != WRONG]
    assert (0, OWN, amounts[OWN], masks[0][OWN]) in hits and (1, OTHER, amounts[OTHER], masks[1][OTHER]) in hits
    assert all(i != TAMPERED for _, i, _, _ in hits)
    pr, cs = TR._split_bytes(B, a, blk7["raw"], blk7["cm"], SCAN_MS, version)
    pr.append(bytes(traw))
    cs.append(bytes(tcm))
    sealed = [FC.pad(MAKER[i], BASE + i) ^ amounts[i] for i in range(len(MS))]
    blk = dict(B=B, bv=bv, raw=b"".join(pr), cm=b"".join(cs), pr=pr, cs=cs, amounts=amounts, verdict=verdict, status=status,
               masks=masks, hits=hits, sealed=sealed)
    _blocks[(cname, amount64, version)] = blk
    return blk


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for blk in TK._blocks.values():
        blk["bv"].close()
    TK._blocks.clear()
    _blocks.clear()


def _both_modes(blk):
    """the two ways to offer amounts: key-major candidates, and one sealed amount per proof"""
    return (dict(amounts=[blk["amounts"]] * len(KEYS)), dict(amounts=blk["sealed"], sealed=True))


@pytest.mark.parametrize("amount64", (False, True))
@pytest.mark.parametrize("cname", CURVES)
def test_block_of_mixed_ownership(cname, amount64):
    """OWN, OTHER, WRONG, DAMAGED, two aggregated proofs, BIG and TAMPERED under three keys: the verdicts are the
    checker's and verify_serialized_mixed's word for word, the hit list is the one ownership gives -- TAMPERED, which the
    plain scan confirms under its owner's key (status 0), is absent.  With key-major amounts and with sealed amounts
    (sealed under each proof's maker key: a foreign key opens another number, which never confirms).  Shuffled, with
    the index as a list."""
    need_gpu()
    blk = _block(cname, amount64, 1)
    bv, raw, cm = blk["bv"], blk["raw"], blk["cm"]
    assert bv.seal_amounts(KEY, [blk["amounts"][i] for i in range(len(MS)) if i != OTHER],
                           index=[BASE + i for i in range(len(MS)) if i != OTHER]).tolist() == \
        [s for i, s in enumerate(blk["sealed"]) if i != OTHER]
    assert bv.seal_amounts(KEY2, [blk["amounts"][OTHER]], index_base=BASE + OTHER).tolist() == [blk["sealed"][OTHER]]
    plain = bv.verify_serialized_mixed(raw, cm, MS, transcript=True)
    assert plain.tolist() == blk["verdict"]
    st, got = bv.scan_serialized_mixed_keys(raw, cm, MS, KEYS, amount64=amount64, index_base=BASE,
                                            amounts=[blk["amounts"]] * len(KEYS))
    assert st.tolist() == blk["status"] and got == blk["masks"] and st[0][TAMPERED] == 0
    for kw in _both_modes(blk):
        ok, hits, found = bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, amount64=amount64, index_base=BASE, **kw)
        assert ok.dtype == np.uint32 and ok.tolist() == blk["verdict"] == plain.tolist()
        assert hits == blk["hits"] and found == len(hits)
    # the flag belongs to the proofs: under the other setting BIG's amount does not open its commitment
    if blk["verdict"][BIG] == 0:
        ok, hits, found = bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, amount64=not amount64, index_base=BASE,
                                                               amounts=blk["sealed"], sealed=True)
        assert ok.tolist() == blk["verdict"] and hits == [h for h in blk["hits"] if h[1] != BIG]
    perm = [5, 0, 7, 6, 3, 1, 4, 2]
    inv = {j: at for at, j in enumerate(perm)}
    want = sorted((kn, inv[i], am, g) for kn, i, am, g in blk["hits"])
    for kw in (dict(amounts=[[blk["amounts"][j] for j in perm]] * len(KEYS)),
               dict(amounts=[blk["sealed"][j] for j in perm], sealed=True)):
        ok, hits, found = bv.verify_find_serialized_mixed_keys(
            b"".join(blk["pr"][j] for j in perm), b"".join(blk["cs"][j] for j in perm), [MS[j] for j in perm], KEYS,
            amount64=amount64, index=[BASE + j for j in perm], **kw)
        assert ok.tolist() == [blk["verdict"][j] for j in perm] and hits == want and found == len(want)


def test_version_2_containers():
    need_gpu()
    blk = _block("bls12_381", True, 2)
    for kw in _both_modes(blk):
        ok, hits, found = blk["bv"].verify_find_serialized_mixed_keys(blk["raw"], blk["cm"], MS, KEYS, uncompressed=True,
                                                                      amount64=True, index_base=BASE, **kw)
        assert ok.tolist() == blk["verdict"] and hits == blk["hits"] and found == len(hits)


@pytest.mark.parametrize("cname", CURVES)
def test_sealed_amounts(cname):
    """seal_amounts is the hashlib pad XOR, over index_base and over an index list, on the host twin and on resident
    buffers (in place too); sealing twice is the identity"""
    torch = need_gpu()
    B, a, bv = TR._engine(cname)
    rng = random.Random(7300 + CID[cname])
    count = 131   # three blocks of lanes, the last one short
    amounts = [0, (1 << 64) - 1, (1 << 31) + 5] + [rng.randrange(1 << 64) for _ in range(count - 3)]
    base = (1 << 32) - 2   # the indices cross 2^32
    index = [rng.randrange(1 << 64) for _ in range(count)]
    for key in (KEY, bytes(32), b"\xff" * 32):
        by_base = bv.seal_amounts(key, amounts, index_base=base)
        assert by_base.dtype == np.uint64 and by_base.tolist() == FC.seal(key, amounts, range(base, base + count))
        by_list = bv.seal_amounts(key, amounts, index=index)
        assert by_list.tolist() == FC.seal(key, amounts, index)
        assert bv.seal_amounts(key, by_base, index_base=base).tolist() == amounts
        assert bv.seal_amounts(key, by_list, index=index).tolist() == amounts
    d_in = TR._dev(torch, np.array(amounts, dtype=np.uint64))
    d_ix = TR._dev(torch, np.array(index, dtype=np.uint64))
    d_out = torch.zeros_like(d_in)
    st = torch.cuda.current_stream().cuda_stream
    bv.seal_amounts_device(KEY, d_in.data_ptr(), count, d_out.data_ptr(), st, d_index=d_ix.data_ptr())
    bv.seal_amounts_device(KEY, d_in.data_ptr(), count, d_in.data_ptr(), st, index_base=base)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().view(np.uint64).tolist() == FC.seal(KEY, amounts, index)
    assert d_in.cpu().numpy().view(np.uint64).tolist() == FC.seal(KEY, amounts, range(base, base + count))
    assert bv.seal_amounts(KEY, []).tolist() == []
    bv.close()


@pytest.mark.parametrize("count", (1, 5))
def test_seal_host_twin_at_one_amount_and_a_few_with_and_without_the_index(count):
    """bpp_amounts_seal on host pointers: the hashlib pad over index_base (index absent) and over an index list"""
    need_gpu()
    B, a, bv = TR._engine("secp256k1")
    amounts = [(1 << 64) - 1, 0, 7, (1 << 31) + 5, 12345][:count]
    index = [(1 << 63) + 9, 3, 0, (1 << 32) - 1, 77][:count]
    base = (1 << 32) - 2
    assert bv.seal_amounts(KEY, amounts, index_base=base).tolist() == FC.seal(KEY, amounts, range(base, base + count))
    assert bv.seal_amounts(KEY, amounts, index=index).tolist() == FC.seal(KEY, amounts, index)
    bv.close()


# ---- order, boundaries and overflow --------------------------------------------------------------------------------------
GRID_COUNT = 683   # 3 x 683 = 2049 pairs: eight compaction blocks of 256 and one pair more
GRID_OWNED = {0: [0, 255, 256], 1: list(range(341, 597)), 2: [100, 682]}


def _grid(cname):
    """683 single outputs under three keys and a fourth that is not in the set.  Pair (j, i) lies at j * 683 + i, a
    compaction block is 256 positions: key 0 owns positions 0, 255 and 256 (first and last of block 0, first of block 1),
    key 1 owns 1024 .. 1279 (all of block 4), key 2 owns 1466 and 2048 (the only pair of block 8); block 2 has none.
    -> (bv, raw, cm, index, amounts, gammas, keys, hits)"""
    r = RC.ORDER[cname]
    assert FC.TILE == 256 and (3 * GRID_COUNT) % 64 != 0
    B, a, bv = TR._engine(cname)
    rng = random.Random(7400 + CID[cname])
    keys = [hashlib.sha256(b"find grid key %d" % j).digest() for j in range(4)]
    owner = [3] * GRID_COUNT
    for j, mine in GRID_OWNED.items():
        for i in mine:
            owner[i] = j
    at = {j * GRID_COUNT + i for j, mine in GRID_OWNED.items() for i in mine}
    assert {0, 255, 256, 2048} <= at and {p // 256 for p in at} == {0, 1, 4, 5, 8} and set(range(1024, 1280)) <= at
    vals = [[rng.randrange(256)] for _ in range(GRID_COUNT)]
    gams = [[rng.randrange(1, r)] for _ in range(GRID_COUNT)]
    pr, cs, index = [None] * GRID_COUNT, [None] * GRID_COUNT, [0] * GRID_COUNT
    for j in range(4):
        mine = [i for i in range(GRID_COUNT) if owner[i] == j]
        raw, cm, ms = bv.prove_serialized_mixed([vals[i] for i in mine], [gams[i] for i in mine], blind_key=keys[j],
                                                transcript=True, index_base=BASE)
        p1, c1 = TR._split_bytes(B, a, raw, cm, [1] * len(mine), 1)
        for t, i in enumerate(mine):
            pr[i], cs[i], index[i] = p1[t], c1[t], BASE + t
    hits = [(j, i, vals[i][0], gams[i][0]) for j in range(3) for i in sorted(GRID_OWNED[j])]
    return bv, b"".join(pr), b"".join(cs), index, [v[0] for v in vals], keys, owner, hits


def _find_device(torch, bv, raw, cm, ms, keys, amounts, index, max_hits, sealed, fill=None):
    """the device entry with guard words behind the records, its workspace as the allocator hands it out or, with `fill`,
    every byte of it set to that value -> (ok, all words of d_hits, n_hits)"""
    count, nk = len(ms), len(keys)
    dev = torch.device("cuda:0")
    d_p = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    d_c = torch.frombuffer(bytearray(cm), dtype=torch.uint8).to(dev)
    d_k = torch.frombuffer(bytearray(b"".join(keys)), dtype=torch.uint8).to(dev)
    d_a = TR._dev(torch, np.array(amounts, dtype=np.uint64).reshape(-1))
    d_ix = TR._dev(torch, np.array(index, dtype=np.uint64))
    d_ok = TR._dev(torch, np.full(count, GUARD, dtype=np.uint32))
    d_hits = TR._dev(torch, np.full((max_hits + 3) * 12, GUARD, dtype=np.uint32))
    d_n = TR._dev(torch, np.full(1, GUARD, dtype=np.uint32))
    wsb = bv.verify_find_workspace_bytes(ms, nk)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    if fill is not None:
        d_ws.fill_(fill)
    bv.verify_find_serialized_mixed_keys_device(d_p.data_ptr(), d_c.data_ptr(), ms, d_k.data_ptr(), nk, d_a.data_ptr(),
                                                d_ok.data_ptr(), d_hits.data_ptr(), max_hits, d_n.data_ptr(), d_ws.data_ptr(),
                                                wsb, torch.cuda.current_stream().cuda_stream, sealed=sealed,
                                                d_index=d_ix.data_ptr())
    torch.cuda.synchronize()
    return (d_ok.cpu().numpy().view(np.uint32).tolist(), d_hits.cpu().numpy().view(np.uint32).reshape(-1, 12),
            int(d_n.cpu().numpy().view(np.uint32)[0]))


def _records(hits):
    out = []
    for j, i, amount, mask in hits:
        out.append([j, i, amount & 0xffffffff, amount >> 32] + [(mask >> (32 * t)) & 0xffffffff for t in range(8)])
    return out


@pytest.mark.parametrize("cname", CURVES)
def test_order_boundaries_and_overflow(cname):
    """the exact ordered list over nine compaction blocks (see _grid); max_hits = 0, 1, n_hits - 1 and n_hits + 3: d_n_hits
    reports all 261, exactly the prefix is written and the words behind it keep their guard value; with no owner among
    the keys nothing is found; under 25 keys the scan of the block counts takes a second step"""
    torch = need_gpu()
    bv, raw, cm, index, amounts, keys, owner, hits = _grid(cname)
    ms = [1] * GRID_COUNT
    n_hits = len(hits)
    assert n_hits == 261 and hits == sorted(hits)
    plain = bv.verify_serialized_mixed(raw, cm, ms, transcript=True).tolist()
    assert plain == [0] * GRID_COUNT
    sealed = [FC.pad(keys[owner[i]], index[i]) ^ amounts[i] for i in range(GRID_COUNT)]
    ok, got, found = bv.verify_find_serialized_mixed_keys(raw, cm, ms, keys[:3], amounts=sealed, sealed=True, index=index)
    assert ok.tolist() == plain and got == hits and found == n_hits
    for max_hits in (0, 1, n_hits - 1, n_hits + 3):
        for sl, am in ((True, sealed), (False, [amounts] * 3)):
            if not sl and max_hits not in (1, n_hits - 1):
                continue
            ok, words, found = _find_device(torch, bv, raw, cm, ms, keys[:3], am, index, max_hits, sl)
            w = min(max_hits, n_hits)
            assert ok == plain and found == n_hits
            assert words[:w].tolist() == _records(hits[:w])
            assert (words[w:] == GUARD).all()
    foreign = [hashlib.sha256(b"nobody %d" % j).digest() for j in range(22)]
    ok, got, found = bv.verify_find_serialized_mixed_keys(raw, cm, ms, foreign[:3], amounts=sealed, sealed=True, index=index)
    assert ok.tolist() == plain and got == [] and found == 0
    # 25 keys, the owners last: 17 075 pairs are 67 compaction blocks, more than the 64 whose counts one step of the scan
    # takes, and key 24's hits (blocks 64 and 66) lie in its second step, behind the 259 of the first
    assert (24 * GRID_COUNT + 100) // FC.TILE == 64 and (25 * GRID_COUNT - 1) // FC.TILE == 66
    ok, got, found = bv.verify_find_serialized_mixed_keys(raw, cm, ms, foreign + keys[:3], amounts=sealed, sealed=True,
                                                          index=index)
    assert ok.tolist() == plain and got == [(22 + j, i, am, g) for j, i, am, g in hits] and found == n_hits
    bv.close()


def _dirty_cases(blk):
    """the block of test 1 whole, and its single outputs alone (no pair word is left to zero then) -> [(positions, ms, raw,
    cm, index, hits by their new positions, the two amount modes as (sealed, amounts))]"""
    out = []
    for pick in (list(range(len(MS))), [i for i, m in enumerate(MS) if m == 1]):
        inv = {i: at for at, i in enumerate(pick)}
        hits = [(j, inv[i], am, g) for j, i, am, g in blk["hits"]]
        assert hits == sorted(hits) and len(hits) == len(blk["hits"])
        modes = ((False, [[blk["amounts"][i] for i in pick]] * len(KEYS)), (True, [blk["sealed"][i] for i in pick]))
        out.append((pick, [MS[i] for i in pick], b"".join(blk["pr"][i] for i in pick), b"".join(blk["cs"][i] for i in pick),
                    [BASE + i for i in pick], hits, modes))
    return out


@pytest.mark.parametrize("cname", CURVES)
def test_workspace_full_of_ones(cname):
    """the device entry over a workspace whose every byte is 0xFF (a fresh allocation is usually zero, and would hide a pair
    word that nothing wrote): the block of test 1 under three keys, max_hits above the hit count, key-major and sealed --
    verdicts, records and n_hits are the fixtures', the words behind the records keep their guard value.  Then the
    block's single outputs alone: every pair word is a kernel's to write, and the call zeroes none."""
    torch = need_gpu()
    blk = _block(cname, False, 1)
    whole, singles = _dirty_cases(blk)
    assert len(whole[0]) == 8 and 1 < len(singles[0]) < 8 and set(singles[1]) == {1}
    for pick, ms, raw, cm, index, want, modes in (whole, singles):
        for sl, am in modes:
            ok, words, found = _find_device(torch, blk["bv"], raw, cm, ms, KEYS, am, index, len(want) + 3, sl, fill=0xff)
            assert ok == [blk["verdict"][i] for i in pick] and found == len(want) > 0
            assert words[:found].tolist() == _records(want) and (words[found:] == GUARD).all()


@pytest.mark.parametrize("cname", CURVES)
def test_agrees_with_the_two_existing_calls(cname):
    """K = 1 and K = 3: d_ok is the verify call's output; the hit list is {(j, i): status[j][i] == 0 and ok[i] == 0} of the
    many-key scan, with its masks"""
    need_gpu()
    blk = _block(cname, False, 1)
    bv, raw, cm = blk["bv"], blk["raw"], blk["cm"]
    ok_v = bv.verify_serialized_mixed(raw, cm, MS, transcript=True)
    for keys in ([KEY], [KEY2], KEYS):
        am = [blk["amounts"]] * len(keys)
        st, masks = bv.scan_serialized_mixed_keys(raw, cm, MS, keys, index_base=BASE, amounts=am)
        want = [(j, i, blk["amounts"][i], masks[j][i]) for j in range(len(keys)) for i in range(len(MS))
                if st[j][i] == 0 and ok_v[i] == 0]
        ok, hits, found = bv.verify_find_serialized_mixed_keys(raw, cm, MS, keys, amounts=am, index_base=BASE)
        assert ok.tolist() == ok_v.tolist() and hits == want and found == len(want)
        assert any(st[j][i] == 0 and ok_v[i] != 0 for j in range(len(keys)) for i in range(len(MS))) == (KEY in keys)


@pytest.mark.parametrize("cname", CURVES)
def test_no_keys_is_still_a_verification(cname):
    """an empty key set over the block of test 1 (a tampered, a damaged and, where the checker says so, an out-of-range
    proof in it): d_ok is the checker's verdicts, never a default, on the host twin and on the device entry with keys,
    amounts and hit records NULL; no hit"""
    torch = need_gpu()
    blk = _block(cname, False, 1)
    bv, raw, cm = blk["bv"], blk["raw"], blk["cm"]
    assert 1 in blk["verdict"] and 2 in blk["verdict"] and 0 in blk["verdict"]
    for kw in (dict(), dict(amounts=blk["sealed"], sealed=True)):
        ok, hits, found = bv.verify_find_serialized_mixed_keys(raw, cm, MS, **kw)
        assert ok.tolist() == blk["verdict"] and hits == [] and found == 0
    dev = torch.device("cuda:0")
    d_p = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    d_c = torch.frombuffer(bytearray(cm), dtype=torch.uint8).to(dev)
    d_ok = TR._dev(torch, np.zeros(len(MS), dtype=np.uint32))   # what a careless caller would read as all Ok
    d_n = TR._dev(torch, np.full(2, GUARD, dtype=np.uint32))
    wsb = bv.verify_find_workspace_bytes(MS, 0)
    assert 0 < wsb <= bv.verify_find_workspace_bytes(MS, 1)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    bv.verify_find_serialized_mixed_keys_device(d_p.data_ptr(), d_c.data_ptr(), MS, 0, 0, 0, d_ok.data_ptr(), 0, 4,
                                                d_n.data_ptr(), d_ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream,
                                                index_base=BASE)
    torch.cuda.synchronize()
    assert d_ok.cpu().numpy().view(np.uint32).tolist() == blk["verdict"]
    assert d_n.cpu().numpy().view(np.uint32).tolist() == [0, GUARD]


@pytest.mark.parametrize("cname", CURVES)
def test_host_twin_at_one_proof_and_the_block_with_and_without_the_optional_inputs(cname):
    """bpp_range_verify_find_serialized_mixed_keys on host pointers at one proof (owned, tampered, aggregated) and at the
    block.  Present: keys, the index list, amounts in both forms, room for the hits -- the checker's verdicts and the hit
    list ownership gives.  Absent: no keys, no index, no amounts, no hit buffer -- the same verdicts, nothing found."""
    need_gpu()
    blk = _block(cname, False, 1)
    bv = blk["bv"]
    for sel in ([OWN], [TAMPERED], [4], list(range(len(MS)))):
        p_, c_, ms_ = b"".join(blk["pr"][j] for j in sel), b"".join(blk["cs"][j] for j in sel), [MS[j] for j in sel]
        verdict = [blk["verdict"][j] for j in sel]
        want = sorted((kn, sel.index(i), am, g) for kn, i, am, g in blk["hits"] if i in sel)
        assert want or sel != [OWN]
        for kw in (dict(amounts=[[blk["amounts"][j] for j in sel]] * len(KEYS)),
                   dict(amounts=[blk["sealed"][j] for j in sel], sealed=True)):
            ok, hits, found = bv.verify_find_serialized_mixed_keys(p_, c_, ms_, KEYS, index=[BASE + j for j in sel], **kw)
            assert ok.tolist() == verdict and hits == want and found == len(want), (sel, kw.get("sealed"))
        ok, hits, found = bv.verify_find_serialized_mixed_keys(p_, c_, ms_, (), index_base=BASE + sel[0], max_hits=0)
        assert ok.tolist() == verdict and hits == [] and found == 0, sel


def test_nothing_to_do_and_errors_that_need_an_engine():
    """count = 0: BPP_OK, d_n_hits[0] = 0 and nothing else written.  A workspace smaller than the layout, an
    m_i above the engine's m: BPP_E_ARG, nothing enqueued, nothing written.  The size grows with the number of keys."""
    torch = need_gpu()
    B, a, bv = TR._engine("secp256k1")
    ok, hits, found = bv.verify_find_serialized_mixed_keys(b"", b"", [], KEYS, amounts=[], sealed=True)
    assert ok.tolist() == [] and hits == [] and found == 0
    ms = [1, 2, 4, 1]
    w1, w3 = bv.verify_find_workspace_bytes(ms, 1), bv.verify_find_workspace_bytes(ms, 3)
    assert 0 < w1 < w3 and bv.verify_find_workspace_bytes([1, 8], 3) == 0
    assert w1 > bv.serialized_mixed_workspace_bytes(ms)
    d = torch.full((4096,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_n = TR._dev(torch, np.full(2, GUARD, dtype=np.uint32))
    p = d.data_ptr()
    d_ws = torch.empty(w3, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for nk in (3, 0):
        d_n[:4] = 0x5a   # the first word back to its guard value
        bv.verify_find_serialized_mixed_keys_device(p, p, [], p, nk, p, p, p, 4, d_n.data_ptr(), d_ws.data_ptr(), w3, st)
        torch.cuda.synchronize()
        assert d_n.cpu().numpy().view(np.uint32).tolist() == [0, GUARD]
    with pytest.raises(B.BppError) as ei:
        bv.verify_find_serialized_mixed_keys_device(p, p, ms, p, 3, p, p, p, 4, d_n.data_ptr(), d_ws.data_ptr(), w3 - 1, st)
    assert ei.value.code == -1 and "workspace too small" in str(ei.value)
    with pytest.raises(B.BppError) as ei:
        bv.verify_find_serialized_mixed_keys_device(p, p, [8, 1], p, 3, p, p, p, 4, d_n.data_ptr(), d_ws.data_ptr(), w3, st)
    assert ei.value.code == -1 and "m_of[0]" in str(ei.value)
    torch.cuda.synchronize()
    assert d.cpu().tolist() == [0x5a] * 4096 and d_n.cpu().numpy().view(np.uint32).tolist() == [0, GUARD]
    bv.close()
