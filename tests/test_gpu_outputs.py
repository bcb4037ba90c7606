"""-m gpu: outputs whose masks are derived from their recipients' keys -- making them (bpp_outputs_make*) and verifying a
block while listing each key's outputs inside aggregated proofs (bpp_range_verify_find_outputs_serialized_mixed_keys*;
csrc/outputs.hpp).

Expected values never come from the library.  Masks, pads and tags are hashlib's (output_cases).  Who owns an output and
its amount are what the test chose.  The verdict of a container is the CHECKER's on the wire record of the same proof
(test_gpu_find._checker_verdict), 2 for the container the test damaged.  The hit list is built from those; the candidate
count is hashlib's."""

import hashlib
import random

import numpy as np
import pytest

import find_cases as FC
import oracle as O
import output_cases as OC
import recover_cases as RC
import tag_cases as TC
import test_gpu_find as TF
import test_gpu_recover as TR
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

CID, CURVES, N, BASE = TR.CID, TR.CURVES, TR.N, TR.BASE
GUARD = TF.GUARD
K0 = hashlib.sha256(b"outputs: scanning key 0").digest()
K1 = hashlib.sha256(b"outputs: scanning key 1").digest()
FOREIGN = hashlib.sha256(b"outputs: a key nobody scans with").digest()
SENDER = hashlib.sha256(b"outputs: the sender's blinding key").digest()

MS = [4, 1, 2, 4, 1, 2, 4]
FIRST = [sum(MS[:i]) for i in range(len(MS))]
N_OUT = sum(MS)
PROOF_OF = [i for i, m in enumerate(MS) for _ in range(m)]
PLACE_OF = [j for m in MS for j in range(m)]
SINGLE, TAMPERED, DAMAGED = 1, 4, 5
O_WRONG_SEALED = FIRST[2]          # (2, 0): K1's, its sealed amount off by one bit: a candidate and no hit
O_FLIPPED_TAG = FIRST[2] + 1       # (2, 1): K0's, one bit of its tag flipped: neither
O_WRONG_PLACE = FIRST[3] + 2       # (3, 2): K0's, its mask derived for j = 1: a candidate and no hit
O_CHANCE = FIRST[6] + 1            # (6, 1): FOREIGN's, and key 2's tag matches it by chance


def _find_key2():
    """a third scanning key whose tag matches FOREIGN's output O_CHANCE by chance: a hashlib search"""
    idx, j = BASE + PROOF_OF[O_CHANCE], PLACE_OF[O_CHANCE]
    want = OC.tag(FOREIGN, idx, j)
    for t in range(1 << 16):
        k = hashlib.sha256(b"outputs: scanning key 2, try %d" % t).digest()
        if OC.tag(k, idx, j) == want:
            return k
    raise AssertionError("no key found")


K2 = _find_key2()
KEYS = [K0, K1, K2]
OWNER = [K0, K1, FOREIGN, K0,   K2,   K1, K0,   K1, FOREIGN, K0, K2,   K0,   K0, K1,   FOREIGN, FOREIGN, K1, K0]
assert len(OWNER) == N_OUT


def _int(words):
    return int.from_bytes(np.ascontiguousarray(words).tobytes(), "little")


def _verdict(cname, n, m, rec, sc):
    """test_gpu_find._checker_verdict at the test's n = 8; the same checker at another n (the C oracle's curves)"""
    if n == N:
        return TF._checker_verdict(cname, m, rec, sc)
    k = TR._k(n, m)
    cp = TR._corpus(cname, n, m)
    O.set_transcript(True)
    try:
        return cp.verdict(rec[:3 + 2 * k], sc, rec[3 + 2 * k:])
    finally:
        O.set_transcript(False)


def _candidates(keys, index, ms, tags, verdict):
    """hashlib: the pairs (key number, output number) of verified proofs whose tag byte is the key's"""
    out, o, rows = [], 0, []
    for i, m in enumerate(ms):
        for j in range(m):
            rows.append((o, i, j))
            o += 1
    for q, k in enumerate(keys):
        for o, i, j in rows:
            if verdict[i] == 0 and OC.tag(k, index[i], j) == tags[o]:
                out.append((q, o))
    return out


_blocks = {}


def _block(cname, amount64, version):
    """the block of mixed ownership -> dict(bv, B, pr, cs (per proof), sealed, tags (per output), amounts, masks (the
    owner's, hashlib), verdict (the checker's), hits [(key_no, output_no, amount, mask)])"""
    key = (cname, amount64, version)
    if key in _blocks:
        return _blocks[key]
    r = RC.ORDER[cname]
    B, a, bv = TR._engine(cname)
    rng = random.Random(8100 + CID[cname])
    amounts = [rng.randrange(1 << N) for _ in range(N_OUT)]
    idx = [BASE + PROOF_OF[o] for o in range(N_OUT)]
    masks = [OC.mask(OWNER[o], idx[o], PLACE_OF[o], r) for o in range(N_OUT)]
    sealed = [amounts[o] ^ OC.pad(OWNER[o], idx[o], PLACE_OF[o]) for o in range(N_OUT)]
    tags = [OC.tag(OWNER[o], idx[o], PLACE_OF[o]) for o in range(N_OUT)]
    # the sender's call gives exactly these
    lm, ls, lt = bv.make_outputs(OWNER, amounts, MS, index_base=BASE)
    assert [_int(x) for x in lm] == masks and ls.tolist() == sealed and lt.tolist() == tags
    # the single output of key 2, sealed and tagged by the EXISTING calls: the j = 0 identity
    o1 = FIRST[SINGLE]
    assert bv.seal_amounts(K2, [amounts[o1]], index_base=BASE + SINGLE).tolist() == [sealed[o1]]
    assert bv.view_tags(K2, 1, index_base=BASE + SINGLE).tolist() == [tags[o1]]
    assert sealed[o1] == amounts[o1] ^ FC.pad(K2, BASE + SINGLE) and tags[o1] == TC.tag(K2, BASE + SINGLE)
    gams = list(masks)
    gams[O_WRONG_PLACE] = OC.mask(K0, idx[O_WRONG_PLACE], 1, r)
    assert PLACE_OF[O_WRONG_PLACE] == 2 and gams[O_WRONG_PLACE] != masks[O_WRONG_PLACE]
    sealed[O_WRONG_SEALED] ^= 1
    tags[O_FLIPPED_TAG] ^= 0x10
    vals = [[amounts[FIRST[i] + j] for j in range(m)] for i, m in enumerate(MS)]
    gm = [[gams[FIRST[i] + j] for j in range(m)] for i, m in enumerate(MS)]
    kw = dict(transcript=True, blind_key=SENDER, index_base=BASE, amount64=amount64)
    raw, cm, ms = bv.prove_serialized_mixed(vals, gm, uncompressed=version == 2, **kw)
    assert ms.tolist() == MS
    recs, sc = bv.prove_batch_mixed(vals, gm, **kw)
    recs, sc = list(recs), [np.array(x) for x in sc]
    pr, cs = TR._split_bytes(B, a, bytes(raw), bytes(cm), MS, version)
    # TAMPERED: r' + 1 in the container and in the checker's triple
    t = bytearray(pr[TAMPERED])
    tail = len(t) - 96
    rp = int.from_bytes(t[tail:tail + 32], "little")
    assert rp == int(O.wire_to_scalars(sc[TAMPERED])[0])
    rp1 = (rp + 1) % r
    t[tail:tail + 32] = rp1.to_bytes(32, "little")
    pr[TAMPERED] = bytes(t)
    sc[TAMPERED][0] = O.scalars_to_wire([rp1])[0]
    bad = bytearray(pr[DAMAGED])
    bad[7] ^= 3   # the header's m
    pr[DAMAGED] = bytes(bad)
    verdict = [2 if i == DAMAGED else _verdict(cname, N, m, recs[i], sc[i]) for i, m in enumerate(MS)]
    assert verdict == [0, 0, 0, 0, 1, 2, 0]
    no_hit = {O_WRONG_SEALED, O_FLIPPED_TAG, O_WRONG_PLACE}
    hits = [(q, o, amounts[o], masks[o]) for q, k in enumerate(KEYS) for o in range(N_OUT)
            if OWNER[o] == k and verdict[PROOF_OF[o]] == 0 and o not in no_hit]
    blk = dict(B=B, bv=bv, pr=pr, cs=cs, sealed=sealed, tags=tags, amounts=amounts, masks=masks, verdict=verdict, hits=hits)
    _blocks[key] = blk
    return blk


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for blk in _blocks.values():
        blk["bv"].close()
    _blocks.clear()


def _per_output(xs, ms, sel):
    """the per-output list xs of a block of shapes ms, for the proofs sel in that order"""
    first = [sum(ms[:i]) for i in range(len(ms))]
    return [xs[first[i] + j] for i in sel for j in range(ms[i])]


def _find_device(torch, bv, raw, cm, ms, keys, sealed, tags, index, max_hits, fill=None):
    """the device entry with guard words behind the records -> (ok, all words of d_hits, n_hits, n_candidates, the
    workspace's bytes after the call)"""
    count, nk = len(ms), len(keys)
    dev = torch.device("cuda:0")
    d_p = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    d_c = torch.frombuffer(bytearray(cm), dtype=torch.uint8).to(dev)
    d_k = torch.frombuffer(bytearray(b"".join(keys)), dtype=torch.uint8).to(dev)
    d_s = TR._dev(torch, np.array(sealed, dtype=np.uint64))
    d_t = TR._dev(torch, np.array(tags, dtype=np.uint8))
    d_ix = TR._dev(torch, np.array(index, dtype=np.uint64))
    d_ok = TR._dev(torch, np.full(count, GUARD, dtype=np.uint32))
    d_hits = TR._dev(torch, np.full((max_hits + 3) * 12, GUARD, dtype=np.uint32))
    d_n = TR._dev(torch, np.full(4, GUARD, dtype=np.uint32))   # [n_hits, guard, n_candidates, guard]
    wsb = bv.verify_find_outputs_workspace_bytes(ms, nk)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    if fill is not None:
        d_ws.fill_(fill)
    bv.verify_find_outputs_serialized_mixed_keys_device(d_p.data_ptr(), d_c.data_ptr(), ms, d_k.data_ptr(), nk, d_s.data_ptr(),
                                                        d_t.data_ptr(), d_ok.data_ptr(), d_hits.data_ptr(), max_hits,
                                                        d_n.data_ptr(), d_ws.data_ptr(), wsb,
                                                        torch.cuda.current_stream().cuda_stream, d_index=d_ix.data_ptr(),
                                                        d_n_candidates=d_n.data_ptr() + 8)
    torch.cuda.synchronize()
    n = d_n.cpu().numpy().view(np.uint32).tolist()
    assert n[1] == n[3] == GUARD
    return (d_ok.cpu().numpy().view(np.uint32).tolist(), d_hits.cpu().numpy().view(np.uint32).reshape(-1, 12), n[0], n[2],
            d_ws.cpu().numpy().tobytes())


# ---- 1. make_outputs is hashlib's -------------------------------------------------------------------------------------------
def _shapes(n_out):
    ms, left = [], n_out
    for m in [4, 1, 2] * n_out:
        if left == 0:
            break
        m = m if m <= left else 1
        ms.append(m)
        left -= m
    return ms


@pytest.mark.parametrize("cname", CURVES)
def test_make_outputs_is_the_hashes(cname):
    """1, 63, 64, 65 and 131 outputs in proofs of 4, 1 and 2, per-output keys drawn from four, the proofs' index crossing
    2^32: masks, sealed amounts and tags are hashlib's, on the host twin and on resident buffers between guard bytes, with
    each output pointer NULL in turn; commit_batch(amounts, masks) gives the checker's commitments"""
    torch = need_gpu()
    B, a, bv = TR._engine(cname)
    r = RC.ORDER[cname]
    cp = TR._corpus(cname, N, TR.CAP)   # the engine's g and h
    rng = random.Random(8000 + CID[cname])
    four = [bytes(32), b"\xff" * 32, K0, FOREIGN]
    base = (1 << 32) - 2
    for n_out in (1, 63, 64, 65, 131):
        ms = _shapes(n_out)
        assert sum(ms) == n_out
        keys = [four[rng.randrange(4)] for _ in range(n_out)]
        amounts = [0, (1 << 64) - 1, (1 << 31) + 5][:n_out] + [rng.randrange(1 << 64) for _ in range(max(0, n_out - 3))]
        pidx = [rng.randrange(1 << 64) for _ in ms]
        for index in (None, pidx):
            ix = [base + i for i in range(len(ms))] if index is None else index
            idx, place = _per_output_index(ix, ms)
            want_m = [OC.mask(keys[o], idx[o], place[o], r) for o in range(n_out)]
            want_s = [amounts[o] ^ OC.pad(keys[o], idx[o], place[o]) for o in range(n_out)]
            want_t = [OC.tag(keys[o], idx[o], place[o]) for o in range(n_out)]
            masks, sealed, tags = bv.make_outputs(keys, amounts, ms, index_base=base, index=index)
            assert masks.dtype == np.uint64 and masks.shape == (n_out, 4) and [_int(x) for x in masks] == want_m
            assert sealed.dtype == np.uint64 and sealed.tolist() == want_s
            assert tags.dtype == np.uint8 and tags.tolist() == want_t
        # resident buffers: 64 guard bytes on either side of each output; each output pointer NULL in turn
        G = 64
        d_k = torch.frombuffer(bytearray(b"".join(keys)), dtype=torch.uint8).to("cuda:0")
        d_ix = TR._dev(torch, np.array(idx, dtype=np.uint64))
        d_j = TR._dev(torch, np.array(place, dtype=np.uint32))
        d_a = TR._dev(torch, np.array(amounts, dtype=np.uint64))
        st = torch.cuda.current_stream().cuda_stream
        for skip in (None, 0, 1, 2):
            outs = [torch.full((G + n_out * w + G,), 0x5a, dtype=torch.uint8, device="cuda:0") for w in (32, 8, 1)]
            ptrs = [0 if t == skip else outs[t].data_ptr() + G for t in range(3)]
            bv.make_outputs_device(d_k.data_ptr(), d_ix.data_ptr(), d_j.data_ptr(), d_a.data_ptr(), n_out, ptrs[0], ptrs[1],
                                   ptrs[2], st)
            torch.cuda.synchronize()
            got = [x.cpu().numpy() for x in outs]
            for t, w in enumerate((32, 8, 1)):
                assert (got[t][:G] == 0x5a).all() and (got[t][G + n_out * w:] == 0x5a).all()
                if t == skip:
                    assert (got[t] == 0x5a).all()
            if skip != 0:
                assert [_int(x) for x in got[0][G:G + n_out * 32].reshape(n_out, 32)] == want_m
            if skip != 1:
                assert got[1][G:G + n_out * 8].copy().view(np.uint64).tolist() == want_s
            if skip != 2:
                assert got[2][G:G + n_out].tolist() == want_t
        if n_out == 65:   # the masks plug into the commitment call: the checker's commitments of a few of them
            small = [am & 0xff for am in amounts]
            V = bv.commit_batch(small, masks)
            for o in (0, 1, 63, 64):
                assert np.array_equal(V[o], cp.commit(small[o], want_m[o])), o
    m0, s0, t0 = bv.make_outputs([], [], [])
    assert m0.shape == (0, 4) and s0.tolist() == [] and t0.tolist() == []
    bv.close()


def _per_output_index(pidx, ms):
    idx, place = [], []
    for i, m in enumerate(ms):
        for j in range(m):
            idx.append(pidx[i] & OC.MASK64)
            place.append(j)
    return idx, place


# ---- 2. the block of mixed ownership ------------------------------------------------------------------------------------------
def _check_block(blk, amount64, **kw):
    bv = blk["bv"]
    raw, cm = b"".join(blk["pr"]), b"".join(blk["cs"])
    index = [BASE + i for i in range(len(MS))]
    cands = _candidates(KEYS, index, MS, blk["tags"], blk["verdict"])
    hit_pairs = [(q, o) for q, o, _, _ in blk["hits"]]
    assert set(hit_pairs) <= set(cands)
    assert (1, O_WRONG_SEALED) in cands and (1, O_WRONG_SEALED) not in hit_pairs
    assert (0, O_WRONG_PLACE) in cands and (0, O_WRONG_PLACE) not in hit_pairs
    assert (2, O_CHANCE) in cands and (2, O_CHANCE) not in hit_pairs
    assert (0, O_FLIPPED_TAG) not in cands
    assert all(PROOF_OF[o] not in (TAMPERED, DAMAGED) for _, o in cands)
    # an m = 4 proof whose outputs belong to key 0, key 1, a foreign key and key 0; key 2's single output
    assert [(q, o) for q, o in hit_pairs if PROOF_OF[o] == 0] == [(0, 0), (0, 3), (1, 1)] and (2, FIRST[SINGLE]) in hit_pairs
    plain = bv.verify_serialized_mixed(raw, cm, MS, transcript=True, **kw)
    assert plain.tolist() == blk["verdict"]
    out = []
    for _ in range(2):   # twice, the same bytes out
        ok, hits, found, n_cand = bv.verify_find_outputs_serialized_mixed_keys(raw, cm, MS, KEYS, blk["sealed"], blk["tags"],
                                                                               amount64=amount64, index_base=BASE, **kw)
        assert ok.dtype == np.uint32 and ok.tolist() == blk["verdict"] == plain.tolist()
        assert hits == blk["hits"] == sorted(hits) and found == len(hits)
        assert n_cand == len(cands)
        out.append((ok.tobytes(), hits, found, n_cand))
    assert out[0] == out[1]
    return cands


@pytest.mark.parametrize("amount64", (False, True))
@pytest.mark.parametrize("cname", CURVES)
def test_block_of_mixed_ownership(cname, amount64):
    """m_of = [4, 1, 2, 4, 1, 2, 4] under three scanning keys, proved by the device prover under a sender key that is none
    of them.  d_ok is the checker's and verify_serialized_mixed's; the hit list is exact with its order, amounts and masks;
    n_candidates is the hashlib count.  Shuffled with the index as a list; twice; max_hits 0, 1, hits - 1 on resident
    buffers with guard words; no non-hit's mask anywhere in the workspace after a device call."""
    torch = need_gpu()
    blk = _block(cname, amount64, 1)
    bv = blk["bv"]
    cands = _check_block(blk, amount64)
    r = RC.ORDER[cname]
    # shuffled, the index as a list
    perm = [5, 0, 6, 3, 1, 4, 2]
    pms = [MS[i] for i in perm]
    new_first = {i: sum(pms[:at]) for at, i in enumerate(perm)}
    renum = lambda o: new_first[PROOF_OF[o]] + PLACE_OF[o]
    want = sorted((q, renum(o), am, g) for q, o, am, g in blk["hits"])
    praw, pcm = b"".join(blk["pr"][i] for i in perm), b"".join(blk["cs"][i] for i in perm)
    pse, ptg = _per_output(blk["sealed"], MS, perm), _per_output(blk["tags"], MS, perm)
    pix = [BASE + i for i in perm]
    ok, hits, found, n_cand = bv.verify_find_outputs_serialized_mixed_keys(praw, pcm, pms, KEYS, pse, ptg, amount64=amount64,
                                                                           index=pix)
    assert ok.tolist() == [blk["verdict"][i] for i in perm] and hits == want and found == len(want) and n_cand == len(cands)
    # resident buffers, guard words past min(found, max_hits) records
    raw, cm = b"".join(blk["pr"]), b"".join(blk["cs"])
    index = [BASE + i for i in range(len(MS))]
    n_hits = len(blk["hits"])
    assert n_hits >= 3
    if amount64:   # the device entry does not depend on the flag's meaning: one setting is enough for the boundaries
        return
    for max_hits in (0, 1, n_hits - 1, n_hits + 2):
        ok, words, found, n_cand, ws = _find_device(torch, bv, raw, cm, MS, KEYS, blk["sealed"], blk["tags"], index, max_hits,
                                                    fill=0xff)
        w = min(max_hits, n_hits)
        assert ok == blk["verdict"] and found == n_hits and n_cand == len(cands)
        assert words[:w].tolist() == TF._records(blk["hits"][:w]) and (words[w:] == GUARD).all()
    # the key rule: the workspace was all ones before the call, so every other byte in it was written by the call -- and
    # no non-hit pair's mask is among them, the owners' of the outputs that are no hit included
    hit_pairs = {(q, o) for q, o, _, _ in blk["hits"]}
    for q, k in enumerate(KEYS):
        for o in range(N_OUT):
            g = OC.mask(k, BASE + PROOF_OF[o], PLACE_OF[o], r).to_bytes(32, "little")
            assert ((q, o) in hit_pairs) == (g in ws), (q, o)
    assert OC.mask(K0, BASE + 3, 1, r).to_bytes(32, "little") not in ws   # the mask O_WRONG_PLACE was committed with


def test_version_2_containers():
    need_gpu()
    _check_block(_block("bls12_381", True, 2), True, uncompressed=True)


@pytest.mark.parametrize("cname", CURVES)
def test_nothing_to_do_and_errors_that_need_an_engine(cname):
    """n_keys = 0: the block verified all the same, on the host twin and on the device entry with keys, sealed amounts, tags
    and records NULL; count = 0; a block of single outputs only; a workspace one byte short; an m_i above the engine's"""
    torch = need_gpu()
    import ctypes

    from bulletproofsplus_amd import _lib
    blk = _block(cname, False, 1)
    B, bv = blk["B"], blk["bv"]
    raw, cm = b"".join(blk["pr"]), b"".join(blk["cs"])
    ok, hits, found, n_cand = bv.verify_find_outputs_serialized_mixed_keys(raw, cm, MS)
    assert ok.tolist() == blk["verdict"] and hits == [] and found == 0 and n_cand == 0
    dev = torch.device("cuda:0")
    d_p = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    d_c = torch.frombuffer(bytearray(cm), dtype=torch.uint8).to(dev)
    d_ok = TR._dev(torch, np.zeros(len(MS), dtype=np.uint32))   # what a careless caller would read as all Ok
    d_n = TR._dev(torch, np.full(4, GUARD, dtype=np.uint32))
    wsb = bv.verify_find_outputs_workspace_bytes(MS, 0)
    assert 0 < wsb < bv.verify_find_outputs_workspace_bytes(MS, 1) < bv.verify_find_outputs_workspace_bytes(MS, 3)
    d_ws = torch.empty(bv.verify_find_outputs_workspace_bytes(MS, 3), dtype=torch.uint8, device=dev)
    m = np.array(MS, dtype=np.uint32)
    st = torch.cuda.current_stream().cuda_stream
    rc = _lib.lib().bpp_range_verify_find_outputs_serialized_mixed_keys_device(
        bv.handle, d_p.data_ptr(), d_c.data_ptr(), m.ctypes.data_as(ctypes.c_void_p), len(MS), 1, None, 0, ctypes.c_uint64(BASE),
        None, None, None, d_ok.data_ptr(), None, 4, d_n.data_ptr(), d_n.data_ptr() + 8, d_ws.data_ptr(), wsb, st or None)
    assert rc == 0
    torch.cuda.synchronize()
    assert d_ok.cpu().numpy().view(np.uint32).tolist() == blk["verdict"]
    assert d_n.cpu().numpy().view(np.uint32).tolist() == [0, GUARD, 0, GUARD]
    # count = 0
    ok, hits, found, n_cand = bv.verify_find_outputs_serialized_mixed_keys(b"", b"", [], KEYS, [], [])
    assert ok.tolist() == [] and hits == [] and found == 0 and n_cand == 0
    d = torch.full((4096,), 0x5a, dtype=torch.uint8, device=dev)
    p = d.data_ptr()
    w3 = bv.verify_find_outputs_workspace_bytes(MS, 3)

    def call(ms_, nk, wsb_):
        bv.verify_find_outputs_serialized_mixed_keys_device(p, p, ms_, p, nk, p, p, p, p, 4, d_n.data_ptr(), d_ws.data_ptr(), wsb_,
                                                            st, d_n_candidates=d_n.data_ptr() + 8)
    for nk in (3, 0):
        d_n[:] = 0x5a
        call([], nk, w3)
        torch.cuda.synchronize()
        assert d_n.cpu().numpy().view(np.uint32).tolist() == [0, GUARD, 0, GUARD]
    # a block of single outputs only: key 2's output and the tampered one
    sel = [SINGLE, TAMPERED]
    ok, hits, found, n_cand = bv.verify_find_outputs_serialized_mixed_keys(
        b"".join(blk["pr"][i] for i in sel), b"".join(blk["cs"][i] for i in sel), [1, 1], KEYS,
        _per_output(blk["sealed"], MS, sel), _per_output(blk["tags"], MS, sel), index=[BASE + i for i in sel])
    o1 = FIRST[SINGLE]
    assert ok.tolist() == [0, 1] and hits == [(2, 0, blk["amounts"][o1], blk["masks"][o1])] and found == 1
    assert n_cand == len(_candidates(KEYS, [BASE + i for i in sel], [1, 1], _per_output(blk["tags"], MS, sel), [0, 1]))
    # errors: nothing enqueued, nothing written
    with pytest.raises(B.BppError) as ei:
        call(MS, 3, w3 - 1)
    assert ei.value.code == -1 and "workspace too small" in str(ei.value)
    with pytest.raises(B.BppError) as ei:
        call([8, 1], 3, w3)
    assert ei.value.code == -1 and "m_of[0]" in str(ei.value)
    assert bv.verify_find_outputs_workspace_bytes([1, 8], 3) == 0
    torch.cuda.synchronize()
    assert d.cpu().tolist() == [0x5a] * 4096 and d_n.cpu().numpy().view(np.uint32).tolist() == [0, GUARD, 0, GUARD]


# ---- 3. tile boundaries -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_tile_boundaries(cname):
    """65 proofs of m = 4, three of m = 1 and one of m = 2 between them: 260 outputs in one class, so the tag test's
    second tile of a key is four positions long.  Owned outputs at class positions 0, 63, 64, 255, 256 and 259, and the
    m = 1 and m = 2 outputs, under three keys; everything else belongs to a key nobody scans with.  The list and the
    counts are exact."""
    need_gpu()
    r = RC.ORDER[cname]
    B, a, bv = TR._engine(cname)
    rng = random.Random(8200 + CID[cname])
    ms = [4] * 65
    for at in (66, 31, 0):   # caller positions of the small proofs: first, in the middle, and near the end
        ms.insert(at, 1)
    ms.insert(40, 2)
    assert len(ms) == 69 and sum(ms) == 265 and ms.count(4) == 65
    index = [BASE + i for i in range(len(ms))]   # the proofs' blinding indices, as the sender used them
    owner, cls4 = [], 0
    by_class_pos = {0: K0, 63: K1, 64: K2, 255: K0, 256: K1, 259: K2}
    singles = iter([K0, K1, K2])
    for m in ms:
        if m == 4:
            owner += [by_class_pos.get(cls4 + j, FOREIGN) for j in range(4)]
            cls4 += 4
        elif m == 1:
            owner.append(next(singles))
        else:
            owner += [K2, K0]
    assert cls4 == 260 and sum(1 for k in owner if k != FOREIGN) == 11
    n_out = len(owner)
    idx, place = _per_output_index(index, ms)
    amounts = [rng.randrange(1 << N) for _ in range(n_out)]
    masks = [OC.mask(owner[o], idx[o], place[o], r) for o in range(n_out)]
    sealed = [amounts[o] ^ OC.pad(owner[o], idx[o], place[o]) for o in range(n_out)]
    tags = [OC.tag(owner[o], idx[o], place[o]) for o in range(n_out)]
    first = [sum(ms[:i]) for i in range(len(ms))]
    vals = [[amounts[first[i] + j] for j in range(m)] for i, m in enumerate(ms)]
    gm = [[masks[first[i] + j] for j in range(m)] for i, m in enumerate(ms)]
    kw = dict(transcript=True, blind_key=SENDER, index_base=BASE)
    raw, cm, _ = bv.prove_serialized_mixed(vals, gm, **kw)
    recs, sc = bv.prove_batch_mixed(vals, gm, **kw)
    verdict = [TF._checker_verdict(cname, m, recs[i], sc[i]) for i, m in enumerate(ms)]
    assert verdict == [0] * len(ms)
    keys = [K0, K1, K2]
    want = [(q, o, amounts[o], masks[o]) for q, k in enumerate(keys) for o in range(n_out) if owner[o] == k]
    cands = _candidates(keys, index, ms, tags, verdict)
    assert len(want) == 11 and len(cands) >= 11
    ok, hits, found, n_cand = bv.verify_find_outputs_serialized_mixed_keys(raw, cm, ms, keys, sealed, tags, index=index)
    assert ok.tolist() == verdict and hits == want and found == 11 and n_cand == len(cands)
    ok, hits, found, n_cand = bv.verify_find_outputs_serialized_mixed_keys(raw, cm, ms, keys[::-1], sealed, tags, index=index,
                                                                           max_hits=5)
    want_r = sorted((2 - q, o, am, g) for q, o, am, g in want)
    assert ok.tolist() == verdict and hits == want_r[:5] and found == 11 and n_cand == len(cands)
    bv.close()


# ---- 5. full-width amounts ----------------------------------------------------------------------------------------------------
def test_full_width_amounts():
    """engine (64, 2): one m = 2 proof over 2^31 + 5 and 2^63 + 9, proved with amount64.  Both outputs are hits with the flag
    and neither without it, while d_ok stays the checker's."""
    need_gpu()
    cname = "secp256k1"
    r = RC.ORDER[cname]
    B, a, bv = TR._engine(cname, n=64, cap=2)
    amounts = [(1 << 31) + 5, (1 << 63) + 9]
    idx = BASE + 3
    masks = [OC.mask(K0, idx, j, r) for j in range(2)]
    sealed = [amounts[j] ^ OC.pad(K0, idx, j) for j in range(2)]
    tags = [OC.tag(K0, idx, j) for j in range(2)]
    kw = dict(transcript=True, blind_key=SENDER, index_base=idx, amount64=True)
    raw, cm, _ = bv.prove_serialized_mixed([amounts], [masks], **kw)
    recs, sc = bv.prove_batch_mixed([amounts], [masks], **kw)
    verdict = [_verdict(cname, 64, 2, recs[0], sc[0])]
    assert verdict == [0]
    ok, hits, found, n_cand = bv.verify_find_outputs_serialized_mixed_keys(raw, cm, [2], [K1, K0], sealed, tags, amount64=True,
                                                                           index_base=idx)
    assert ok.tolist() == verdict and hits == [(1, 0, amounts[0], masks[0]), (1, 1, amounts[1], masks[1])] and found == 2
    assert n_cand == len(_candidates([K1, K0], [idx], [2], tags, verdict))
    ok, hits, found, n_cand2 = bv.verify_find_outputs_serialized_mixed_keys(raw, cm, [2], [K1, K0], sealed, tags, index_base=idx)
    assert ok.tolist() == verdict and hits == [] and found == 0 and n_cand2 == n_cand
    bv.close()
