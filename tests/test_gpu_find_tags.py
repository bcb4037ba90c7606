"""-m gpu: view tags, and the verify-and-find call that tests them first (bpp_view_tags*,
bpp_range_verify_find_tagged_serialized_mixed_keys*; csrc/find.hpp).

Expected values never come from the library.  The tag of an output is hashlib's (tag_cases.tag), made under the key of
whoever made the proof.  The verdicts, the owners and the hit lists are those of tests/test_gpu_find.py, whose blocks are
reused by import: a candidate is a pair whose proof is a verified single output and whose tag byte is the key's, counted
with hashlib; a hit is a hit of the untagged call among the candidates."""

import hashlib
import random

import numpy as np
import pytest

import find_cases as FC
import tag_cases as TC
import test_gpu_find as TF
import test_gpu_recover as TR
import test_gpu_recover_keys as TK
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

CID, CURVES, BASE = TR.CID, TR.CURVES, TR.BASE
KEY, KEY2, KEYS = TK.KEY, TK.KEY2, TK.KEYS
MS, MAKER, GUARD = TF.MS, TF.MAKER, TF.GUARD
OWN, OTHER, WRONG, DAMAGED, BIG, TAMPERED = TF.OWN, TF.OTHER, TF.WRONG, TF.DAMAGED, TF.BIG, TF.TAMPERED
INDEX = [BASE + i for i in range(len(MS))]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for blk in TK._blocks.values():
        blk["bv"].close()
    TK._blocks.clear()
    TF._blocks.clear()


def _maker_tags():
    """the byte each container of test_gpu_find._block carries: its maker's (aggregated proofs carry one too; it is not read)"""
    return [TC.tag(MAKER[i], INDEX[i]) for i in range(len(MS))]


def _eligible(blk):
    """a candidate's proof: a single output the checker accepts (which the decoder then took, with non-zero challenges)"""
    return [MS[i] == 1 and blk["verdict"][i] == 0 for i in range(len(MS))]


def _tagged_hits(blk, keys, tags):
    """the hits of the untagged call among the candidates of `tags`, with key numbers in `keys`"""
    cands = TC.candidates(keys, INDEX, tags, _eligible(blk))
    hits = []
    for j, k in enumerate(keys):
        for kn, i, am, g in blk["hits"]:
            if KEYS[kn] == k and (j, i) in cands:
                hits.append((j, i, am, g))
    return cands, sorted(hits)


# ---- 1. tags are the hash ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_tags_are_the_hash(cname):
    """view_tags is hashlib's byte over index_base (crossing 2^32) and over a list of random u64, for the all-zero, the
    all-ones and a random key, at 1, 63, 64, 65 and 131 outputs (the last lanes of a block, one block and one lane more,
    three blocks); on the host twin and on resident buffers; count = 0"""
    torch = need_gpu()
    B, a, bv = TR._engine(cname)
    rng = random.Random(7700 + CID[cname])
    base = (1 << 32) - 2
    for count in (1, 63, 64, 65, 131):
        index = [rng.randrange(1 << 64) for _ in range(count)]
        for key in (KEY, bytes(32), b"\xff" * 32):
            by_base = bv.view_tags(key, count, index_base=base)
            assert by_base.dtype == np.uint8 and by_base.tolist() == TC.tags(key, range(base, base + count))
            assert bv.view_tags(key, index=index).tolist() == TC.tags(key, index)
        d_ix = TR._dev(torch, np.array(index, dtype=np.uint64))
        d_out = TR._dev(torch, np.full(count + 8, 0x5a, dtype=np.uint8))
        d_out2 = TR._dev(torch, np.full(count + 8, 0x5a, dtype=np.uint8))
        st = torch.cuda.current_stream().cuda_stream
        bv.view_tags_device(KEY, count, d_out.data_ptr(), st, d_index=d_ix.data_ptr())
        bv.view_tags_device(KEY, count, d_out2.data_ptr(), st, index_base=base)
        torch.cuda.synchronize()
        assert d_out.cpu().tolist() == TC.tags(KEY, index) + [0x5a] * 8
        assert d_out2.cpu().tolist() == TC.tags(KEY, range(base, base + count)) + [0x5a] * 8
    assert bv.view_tags(KEY, 0).tolist() == [] and bv.view_tags(KEY, index=[]).tolist() == []
    bv.view_tags_device(KEY, 0, 0)
    bv.close()


# ---- 2. the mixed-ownership block -------------------------------------------------------------------------------------
def _check_block(blk, amount64, **kw):
    bv, raw, cm = blk["bv"], blk["raw"], blk["cm"]
    tags = _maker_tags()
    cands, want = _tagged_hits(blk, KEYS, tags)
    assert want == blk["hits"]   # true tags remove no hit
    assert (0, WRONG) in cands and all(i not in (TAMPERED, DAMAGED) and MS[i] == 1 for _, i in cands)
    assert (0, WRONG) not in [(j, i) for j, i, _, _ in want]
    plain = bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, amount64=amount64, index_base=BASE,
                                                 amounts=blk["sealed"], sealed=True, **kw)
    for mode in TF._both_modes(blk):
        ok, hits, found, n_cand = bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, amount64=amount64, index_base=BASE,
                                                                       tags=tags, **mode, **kw)
        assert ok.dtype == np.uint32 and ok.tolist() == blk["verdict"] == plain[0].tolist()
        assert hits == blk["hits"] == plain[1] and found == len(hits)
        assert n_cand == len(cands)
    return tags, cands


@pytest.mark.parametrize("amount64", (False, True))
@pytest.mark.parametrize("cname", CURVES)
def test_block_of_mixed_ownership(cname, amount64):
    """OWN, OTHER, WRONG, DAMAGED, two aggregated proofs, BIG and TAMPERED under three keys, tags made under each proof's
    maker: d_ok is the untagged call's word for word, the hits are the block's, n_candidates is the hashlib count -- it has
    (key 0, WRONG), a candidate that is no hit, and neither TAMPERED nor DAMAGED.  Key-major and sealed amounts.  The
    other setting of amount64.  Shuffled, with the index as a list."""
    need_gpu()
    blk = TF._block(cname, amount64, 1)
    bv = blk["bv"]
    tags, cands = _check_block(blk, amount64)
    if blk["verdict"][BIG] == 0:
        ok, hits, found, n_cand = bv.verify_find_serialized_mixed_keys(blk["raw"], blk["cm"], MS, KEYS, amount64=not amount64,
                                                                       index_base=BASE, amounts=blk["sealed"], sealed=True, tags=tags)
        assert ok.tolist() == blk["verdict"] and hits == [h for h in blk["hits"] if h[1] != BIG] and n_cand == len(cands)
    perm = [5, 0, 7, 6, 3, 1, 4, 2]
    inv = {j: at for at, j in enumerate(perm)}
    want = sorted((kn, inv[i], am, g) for kn, i, am, g in blk["hits"])
    for kw in (dict(amounts=[[blk["amounts"][j] for j in perm]] * len(KEYS)),
               dict(amounts=[blk["sealed"][j] for j in perm], sealed=True)):
        ok, hits, found, n_cand = bv.verify_find_serialized_mixed_keys(
            b"".join(blk["pr"][j] for j in perm), b"".join(blk["cs"][j] for j in perm), [MS[j] for j in perm], KEYS,
            amount64=amount64, index=[BASE + j for j in perm], tags=[tags[j] for j in perm], **kw)
        assert ok.tolist() == [blk["verdict"][j] for j in perm] and hits == want and found == len(want)
        assert n_cand == len(cands)


def test_version_2_containers():
    need_gpu()
    _check_block(TF._block("bls12_381", True, 2), True, uncompressed=True)


# ---- 3. the tag decides -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_the_tag_decides(cname):
    """one bit of OWN's tag flipped: OWN leaves the list, nothing else changes; OTHER (made under KEY2) given KEY's byte:
    key 0 gains a candidate and no hit, key 1 loses OTHER unless the two bytes coincide; all tags wrong: no candidate, no
    hit; the same key three times: every owned pair a candidate three times over.  d_ok never moves."""
    need_gpu()
    blk = TF._block(cname, False, 1)
    bv, raw, cm = blk["bv"], blk["raw"], blk["cm"]
    true = _maker_tags()
    true_cands, _ = _tagged_hits(blk, KEYS, true)

    def run(keys, tags, **kw):
        mode = kw or dict(amounts=blk["sealed"], sealed=True)
        return bv.verify_find_serialized_mixed_keys(raw, cm, MS, keys, index_base=BASE, tags=tags, **mode)
    # a flipped bit
    flipped = list(true)
    flipped[OWN] ^= 0x10
    cands, want = _tagged_hits(blk, KEYS, flipped)
    assert want == [h for h in blk["hits"] if h[:2] != (0, OWN)] and len(want) == len(blk["hits"]) - 1
    ok, hits, found, n_cand = run(KEYS, flipped)
    assert ok.tolist() == blk["verdict"] and hits == want and found == len(want) and n_cand == len(cands)
    # OTHER under the wrong key's byte
    swapped = list(true)
    swapped[OTHER] = TC.tag(KEY, INDEX[OTHER])
    coincide = swapped[OTHER] == true[OTHER]
    cands, want = _tagged_hits(blk, KEYS, swapped)
    assert (0, OTHER) in cands and ((1, OTHER) in cands) == coincide
    assert want == [h for h in blk["hits"] if coincide or h[:2] != (1, OTHER)]
    assert set(cands) == (set(true_cands) | {(0, OTHER)}) - (set() if coincide else {(1, OTHER)})
    for mode in TF._both_modes(blk):
        ok, hits, found, n_cand = run(KEYS, swapped, **mode)
        assert ok.tolist() == blk["verdict"] and hits == want and found == len(want) and n_cand == len(cands)
    # every tag wrong for every key of the set
    wrong = []
    for i in range(len(MS)):
        mine = {TC.tag(k, INDEX[i]) for k in KEYS}
        wrong.append(next(b for b in range(256) if b not in mine))
    ok, hits, found, n_cand = run(KEYS, wrong)
    assert ok.tolist() == blk["verdict"] and hits == [] and found == 0 and n_cand == 0
    # the dense list: one key three times
    same = [KEY] * 3
    cands, want = _tagged_hits(blk, same, true)
    mine = [h for h in blk["hits"] if h[0] == 0]
    assert want == [(j, i, am, g) for j in range(3) for _, i, am, g in mine] and len(cands) % 3 == 0
    assert len(cands) == 3 * sum(1 for j, _ in true_cands if j == 0) > len(want)
    for mode in (dict(amounts=[blk["amounts"]] * 3), dict(amounts=blk["sealed"], sealed=True)):
        ok, hits, found, n_cand = run(same, true, **mode)
        assert ok.tolist() == blk["verdict"] and hits == want and found == len(want) and n_cand == len(cands)


# ---- 4. order and boundaries ------------------------------------------------------------------------------------------
def _find_device(torch, bv, raw, cm, ms, keys, amounts, index, tags, max_hits, sealed, fill=None):
    """the device entry with tags and guard words behind the records, its workspace as the allocator hands it out or, with
    `fill`, every byte of it set to that value -> (ok, all words of d_hits, n_hits, n_candidates)"""
    count, nk = len(ms), len(keys)
    dev = torch.device("cuda:0")
    d_p = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    d_c = torch.frombuffer(bytearray(cm), dtype=torch.uint8).to(dev)
    d_k = torch.frombuffer(bytearray(b"".join(keys)), dtype=torch.uint8).to(dev)
    d_a = TR._dev(torch, np.array(amounts, dtype=np.uint64).reshape(-1))
    d_ix = TR._dev(torch, np.array(index, dtype=np.uint64))
    d_t = TR._dev(torch, np.array(tags, dtype=np.uint8))
    d_ok = TR._dev(torch, np.full(count, GUARD, dtype=np.uint32))
    d_hits = TR._dev(torch, np.full((max_hits + 3) * 12, GUARD, dtype=np.uint32))
    d_n = TR._dev(torch, np.full(4, GUARD, dtype=np.uint32))   # [n_hits, guard, n_candidates, guard]
    wsb = bv.verify_find_tagged_workspace_bytes(ms, nk)
    assert wsb >= bv.verify_find_workspace_bytes(ms, nk) > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    if fill is not None:
        d_ws.fill_(fill)
    bv.verify_find_serialized_mixed_keys_device(d_p.data_ptr(), d_c.data_ptr(), ms, d_k.data_ptr(), nk, d_a.data_ptr(),
                                                d_ok.data_ptr(), d_hits.data_ptr(), max_hits, d_n.data_ptr(), d_ws.data_ptr(),
                                                wsb, torch.cuda.current_stream().cuda_stream, sealed=sealed,
                                                d_index=d_ix.data_ptr(), d_tags=d_t.data_ptr(), d_n_candidates=d_n.data_ptr() + 8)
    torch.cuda.synchronize()
    n = d_n.cpu().numpy().view(np.uint32).tolist()
    assert n[1] == n[3] == GUARD
    return (d_ok.cpu().numpy().view(np.uint32).tolist(), d_hits.cpu().numpy().view(np.uint32).reshape(-1, 12), n[0], n[2])


@pytest.mark.parametrize("cname", CURVES)
def test_workspace_full_of_ones(cname):
    """test_gpu_find's test of the same name through the tagged device entry: over a workspace of 0xFF bytes every pair
    that is no candidate must read as no hit, so the call has to zero the pair words whatever the block holds -- the whole
    block of test 1, then its single outputs alone.  Verdicts, records, n_hits and n_candidates (the hashlib count) are the
    fixtures'."""
    torch = need_gpu()
    blk = TF._block(cname, False, 1)
    tags = _maker_tags()
    cands, hits = _tagged_hits(blk, KEYS, tags)
    assert hits == blk["hits"] and 0 < len(hits) < len(cands) < len(KEYS) * len(MS)
    for pick, ms, raw, cm, index, want, modes in TF._dirty_cases(blk):
        for sl, am in modes:
            ok, words, found, n_cand = _find_device(torch, blk["bv"], raw, cm, ms, KEYS, am, index, [tags[i] for i in pick],
                                                    len(want) + 3, sl, fill=0xff)
            assert ok == [blk["verdict"][i] for i in pick] and found == len(want) and n_cand == len(cands)
            assert words[:found].tolist() == TF._records(want) and (words[found:] == GUARD).all()


def _grid_tags(keys_in_set, all_keys, owner, index, need_foreign):
    """the owners' tags over the grid, and the hashlib candidates under keys_in_set.  Outputs of the fourth key (which is in
    no set, so they are never hits) have their byte adjusted where the seed does not give what the test is about: a chance
    match of a key that owns nothing (need_foreign), and a candidate count that is no multiple of 8."""
    count = len(owner)
    tags = [TC.tag(all_keys[owner[i]], index[i]) for i in range(count)]
    owned = {j: {i for i in range(count) if all_keys[owner[i]] == k} for j, k in enumerate(keys_in_set)}
    spare = [i for i in range(count) if owner[i] == 3]

    def cands():
        return TC.candidates(keys_in_set, index, tags, [True] * count)
    if need_foreign and not any(i not in owned[j] for j, i in cands()):
        i = spare.pop()
        tags[i] = TC.tag(keys_in_set[0], index[i])
    if len(cands()) % 8 == 0:
        i = next(i for i in spare if all(TC.tag(k, index[i]) != tags[i] for k in keys_in_set))
        tags[i] = TC.tag(keys_in_set[-1], index[i])
    c = cands()
    assert len(c) % 8 != 0 and (not need_foreign or any(i not in owned[j] for j, i in c))
    return tags, c


@pytest.mark.parametrize("cname", CURVES)
def test_order_boundaries_and_overflow(cname):
    """test_gpu_find._grid: 683 single outputs, nine compaction tiles, tags made by the owners.  Under 3 keys and under 25
    with the owners last (17 075 pairs: the tile scan takes a second step, for the tag test's 75 tiles too): the hits are
    exactly the ordered 261, n_candidates the hashlib count with its chance matches.  Key 1's 256 contiguous owners cross
    a tile edge of its row (positions 341 .. 596, edge at 512); the count is no multiple of 8, so the list kernel's last
    group is short.  Through the device entry with guard words, max_hits = 0, 1, n_hits - 1, n_hits + 3: exactly the
    prefix is written."""
    torch = need_gpu()
    bv, raw, cm, index, amounts, keys, owner, hits = TF._grid(cname)
    count = TF.GRID_COUNT
    ms = [1] * count
    n_hits = len(hits)
    assert n_hits == 261 and hits == sorted(hits) and 341 // FC.TILE != 596 // FC.TILE
    sealed = [FC.pad(keys[owner[i]], index[i]) ^ amounts[i] for i in range(count)]
    tags3, cands3 = _grid_tags(keys[:3], keys, owner, index, False)
    assert {(j, i) for j, i, _, _ in hits} <= set(cands3)
    ok, got, found, n_cand = bv.verify_find_serialized_mixed_keys(raw, cm, ms, keys[:3], amounts=sealed, sealed=True, index=index,
                                                                  tags=tags3)
    assert ok.tolist() == [0] * count and got == hits and found == n_hits and n_cand == len(cands3)
    for max_hits in (0, 1, n_hits - 1, n_hits + 3):
        for sl, am in ((True, sealed), (False, [amounts] * 3)):
            if not sl and max_hits not in (1, n_hits - 1):
                continue
            ok, words, found, n_cand = _find_device(torch, bv, raw, cm, ms, keys[:3], am, index, tags3, max_hits, sl)
            w = min(max_hits, n_hits)
            assert ok == [0] * count and found == n_hits and n_cand == len(cands3)
            assert words[:w].tolist() == TF._records(hits[:w])
            assert (words[w:] == GUARD).all()
    foreign = [hashlib.sha256(b"nobody %d" % j).digest() for j in range(22)]
    set25 = foreign + keys[:3]
    tags25, cands25 = _grid_tags(set25, keys, owner, index, True)
    assert len(cands25) > n_hits and FC.TILE * 64 < 25 * count
    ok, got, found, n_cand = bv.verify_find_serialized_mixed_keys(raw, cm, ms, set25, amounts=sealed, sealed=True, index=index,
                                                                  tags=tags25)
    assert ok.tolist() == [0] * count and got == [(22 + j, i, am, g) for j, i, am, g in hits] and found == n_hits
    assert n_cand == len(cands25)
    ok, words, found, n_cand = _find_device(torch, bv, raw, cm, ms, set25, sealed, index, tags25, n_hits + 3, True)
    assert found == n_hits and n_cand == len(cands25) and (words[n_hits:] == GUARD).all()
    assert words[:n_hits].tolist() == TF._records([(22 + j, i, am, g) for j, i, am, g in hits])
    bv.close()


# ---- 5. agreement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_agrees_with_the_untagged_call(cname):
    """K = 1 and K = 3 with the true tags: the hits and d_ok of the untagged call"""
    need_gpu()
    blk = TF._block(cname, False, 1)
    bv, raw, cm = blk["bv"], blk["raw"], blk["cm"]
    tags = _maker_tags()
    for keys in ([KEY], [KEY2], KEYS):
        for mode in (dict(amounts=[blk["amounts"]] * len(keys)), dict(amounts=blk["sealed"], sealed=True)):
            ok0, hits0, found0 = bv.verify_find_serialized_mixed_keys(raw, cm, MS, keys, index_base=BASE, **mode)
            ok, hits, found, n_cand = bv.verify_find_serialized_mixed_keys(raw, cm, MS, keys, index_base=BASE, tags=tags, **mode)
            assert ok.tolist() == ok0.tolist() == blk["verdict"] and hits == hits0 and found == found0
            assert n_cand == len(TC.candidates(keys, INDEX, tags, _eligible(blk))) >= found
        assert (len(hits0) > 0) == (KEY in keys or KEY2 in keys)


# ---- 6. nothing to do, and errors -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_no_keys_is_still_a_verification(cname):
    """an empty key set: d_ok is the checker's verdicts, never a default, on the host twin and on the device entry with
    keys, amounts, tags and hit records NULL (the tagged entry called directly: the wrapper takes d_tags = 0 for the
    untagged one); no hit, no candidate"""
    torch = need_gpu()
    import ctypes

    from bulletproofsplus_amd import _lib
    blk = TF._block(cname, False, 1)
    bv, raw, cm = blk["bv"], blk["raw"], blk["cm"]
    assert 1 in blk["verdict"] and 2 in blk["verdict"] and 0 in blk["verdict"]
    ok, hits, found, n_cand = bv.verify_find_serialized_mixed_keys(raw, cm, MS, tags=_maker_tags())
    assert ok.tolist() == blk["verdict"] and hits == [] and found == 0 and n_cand == 0
    dev = torch.device("cuda:0")
    d_p = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    d_c = torch.frombuffer(bytearray(cm), dtype=torch.uint8).to(dev)
    d_ok = TR._dev(torch, np.zeros(len(MS), dtype=np.uint32))   # what a careless caller would read as all Ok
    d_n = TR._dev(torch, np.full(4, GUARD, dtype=np.uint32))
    wsb = bv.verify_find_tagged_workspace_bytes(MS, 0)
    assert 0 < wsb <= bv.verify_find_tagged_workspace_bytes(MS, 1)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    m = np.array(MS, dtype=np.uint32)
    rc = _lib.lib().bpp_range_verify_find_tagged_serialized_mixed_keys_device(
        bv.handle, d_p.data_ptr(), d_c.data_ptr(), m.ctypes.data_as(ctypes.c_void_p), len(MS), 1, None, 0, ctypes.c_uint64(BASE),
        None, None, d_ok.data_ptr(), None, 4, d_n.data_ptr(), None, d_n.data_ptr() + 8, d_ws.data_ptr(), wsb,
        torch.cuda.current_stream().cuda_stream or None)
    assert rc == 0
    torch.cuda.synchronize()
    assert d_ok.cpu().numpy().view(np.uint32).tolist() == blk["verdict"]
    assert d_n.cpu().numpy().view(np.uint32).tolist() == [0, GUARD, 0, GUARD]
    # nothing but aggregated proofs, with keys: verified, nothing listed
    agg = [i for i in range(len(MS)) if MS[i] > 1]
    ok, hits, found, n_cand = bv.verify_find_serialized_mixed_keys(
        b"".join(blk["pr"][i] for i in agg), b"".join(blk["cs"][i] for i in agg), [MS[i] for i in agg], KEYS,
        amounts=[0] * len(agg), sealed=True, index=[INDEX[i] for i in agg], tags=[0] * len(agg))
    assert ok.tolist() == [blk["verdict"][i] for i in agg] and hits == [] and found == 0 and n_cand == 0


@pytest.mark.parametrize("cname", CURVES)
def test_host_twin_at_one_proof_and_the_block_with_and_without_the_optional_inputs(cname):
    """bpp_range_verify_find_tagged_serialized_mixed_keys on host pointers at one proof (owned, tampered, aggregated) and at
    the block.  Present: keys, tags, the index list, amounts in both forms, room for the hits -- the checker's verdicts,
    ownership's hits, hashlib's candidate count.  Absent keys (so no tags, no amounts, no index, no hit buffer are read):
    the same verdicts, nothing found, no candidate."""
    need_gpu()
    blk = TF._block(cname, False, 1)
    bv = blk["bv"]
    tags = _maker_tags()
    cands, _ = _tagged_hits(blk, KEYS, tags)
    for sel in ([OWN], [TAMPERED], [4], list(range(len(MS)))):
        p_, c_, ms_ = b"".join(blk["pr"][j] for j in sel), b"".join(blk["cs"][j] for j in sel), [MS[j] for j in sel]
        verdict = [blk["verdict"][j] for j in sel]
        want = sorted((kn, sel.index(i), am, g) for kn, i, am, g in blk["hits"] if i in sel)
        n_want = len([1 for _, i in cands if i in sel])
        for kw in (dict(amounts=[[blk["amounts"][j] for j in sel]] * len(KEYS)),
                   dict(amounts=[blk["sealed"][j] for j in sel], sealed=True)):
            ok, hits, found, n_cand = bv.verify_find_serialized_mixed_keys(p_, c_, ms_, KEYS, index=[BASE + j for j in sel],
                                                                           tags=[tags[j] for j in sel], **kw)
            assert ok.tolist() == verdict and hits == want and found == len(want) and n_cand == n_want, (sel, kw.get("sealed"))
        ok, hits, found, n_cand = bv.verify_find_serialized_mixed_keys(p_, c_, ms_, (), index_base=BASE + sel[0], max_hits=0,
                                                                       tags=[tags[j] for j in sel])
        assert ok.tolist() == verdict and hits == [] and found == 0 and n_cand == 0, sel


def test_nothing_to_do_and_errors_that_need_an_engine():
    """count = 0: BPP_OK, d_n_hits[0] = d_n_candidates[0] = 0 and nothing else written.  A workspace one byte short, an m_i
    above the engine's m: BPP_E_ARG, nothing enqueued, nothing written.  The size is the untagged one and the candidates'
    room."""
    torch = need_gpu()
    B, a, bv = TR._engine("secp256k1")
    ok, hits, found, n_cand = bv.verify_find_serialized_mixed_keys(b"", b"", [], KEYS, amounts=[], sealed=True, tags=[])
    assert ok.tolist() == [] and hits == [] and found == 0 and n_cand == 0
    ms = [1, 2, 4, 1]
    w1, w3 = bv.verify_find_tagged_workspace_bytes(ms, 1), bv.verify_find_tagged_workspace_bytes(ms, 3)
    assert 0 < w1 < w3 and bv.verify_find_tagged_workspace_bytes([1, 8], 3) == 0 == bv.verify_find_workspace_bytes([1, 8], 3)
    assert w3 > bv.verify_find_workspace_bytes(ms, 3) and w3 == bv.verify_find_tagged_workspace_bytes(ms, 3)
    d = torch.full((4096,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_n = TR._dev(torch, np.full(4, GUARD, dtype=np.uint32))
    p = d.data_ptr()
    d_ws = torch.empty(w3, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream

    def call(ms_, nk, wsb):
        bv.verify_find_serialized_mixed_keys_device(p, p, ms_, p, nk, p, p, p, 4, d_n.data_ptr(), d_ws.data_ptr(), wsb, st,
                                                    d_tags=p, d_n_candidates=d_n.data_ptr() + 8)
    for nk in (3, 0):
        d_n[:] = 0x5a
        call([], nk, w3)
        torch.cuda.synchronize()
        assert d_n.cpu().numpy().view(np.uint32).tolist() == [0, GUARD, 0, GUARD]
    with pytest.raises(B.BppError) as ei:
        call(ms, 3, w3 - 1)
    assert ei.value.code == -1 and "workspace too small" in str(ei.value)
    with pytest.raises(B.BppError) as ei:
        call([8, 1], 3, w3)
    assert ei.value.code == -1 and "m_of[0]" in str(ei.value)
    torch.cuda.synchronize()
    assert d.cpu().tolist() == [0x5a] * 4096 and d_n.cpu().numpy().view(np.uint32).tolist() == [0, GUARD, 0, GUARD]
    bv.close()
