"""-m gpu: scanning a block of containers under many keys in one call (bpp_range_scan_serialized_mixed_keys*;
csrc/recover_keys.hpp).

Expected values never come from the library.  Gamma of a (key, proof) pair is recover_cases.recover_bigint on
oracle.blinding_from_key(key, index, k, r), the proof's delta' and the challenge block the CHECKER drew from its wire record
(the C oracle's verifier, pyref on edwards25519 -- test_gpu_recover._checker_challenges); for the owning key it is also
recover_cases.gamma_of from the gammas the test chose.  The status of a pair follows from who made the proof and which
amount the test offers.  The blocks are the device prover's, as in tests/test_gpu_recover.py."""

import hashlib
import random

import numpy as np
import pytest

import oracle as O
import recover_cases as RC
import test_gpu_recover as TR
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

CID, CURVES, N, BASE = TR.CID, TR.CURVES, TR.N, TR.BASE
KEY, KEY2 = TR.KEY, TR.KEY2
KEY3 = hashlib.sha256(b"a key that owns nothing").digest()
KEYS = [KEY, KEY2, KEY3]
SCAN_MS, OWN, OTHER, WRONG, DAMAGED, BIG = TR.SCAN_MS, TR.OWN, TR.OTHER, TR.WRONG, TR.DAMAGED, TR.BIG


def _k(n, m):
    return (n * m).bit_length() - 1


def _gamma_bigint(cname, n, m, sc, ch, key, index):
    """Gamma of one (key, proof) pair by the big-integer formula; ch: the challenges the checker drew from the wire record"""
    r = RC.ORDER[cname]
    return RC.recover_bigint(r, n, m, int(O.wire_to_scalars(sc)[2]), ch, O.blinding_from_key(key, index, _k(n, m), r))


_blocks = {}


def _block(cname, amount64, version):
    """test_gpu_recover._scan_block's block -- made under KEY at BASE + i, container OTHER the same output proved under KEY2,
    WRONG with another candidate amount, DAMAGED with a flipped header byte, BIG an amount of 2^31 + 5 -- with what a scan
    under KEYS must answer: -> dict(bv, B, raw, cm, amounts, status (3 x 7), masks (3 x 7), gamma (3 x 7, by big integers))"""
    if (cname, amount64, version) in _blocks:
        return _blocks[(cname, amount64, version)]
    r = RC.ORDER[cname]
    B, a, bv = TR._engine(cname)
    vals, gams = TR._inputs(cname, SCAN_MS, N, 5500 + CID[cname])
    vals[BIG] = [TR.BIG_AMOUNT]
    kw = dict(transcript=True, index_base=BASE, uncompressed=version == 2, amount64=amount64)
    raw, cm, ms = bv.prove_serialized_mixed(vals, gams, blind_key=KEY, **kw)
    raw2, cm2, _ = bv.prove_serialized_mixed(vals, gams, blind_key=KEY2, **kw)
    assert ms.tolist() == SCAN_MS and cm == cm2
    pr, cs = TR._split_bytes(B, a, raw, cm, SCAN_MS, version)
    pr2, _ = TR._split_bytes(B, a, raw2, cm2, SCAN_MS, version)
    pr[OTHER] = pr2[OTHER]
    bad = bytearray(pr[DAMAGED])
    bad[7] ^= 3   # the header's m
    pr[DAMAGED] = bytes(bad)
    amounts = [v[0] for v in vals]
    amounts[WRONG] += 1
    # the wire records of the same proofs, for the checker
    wkw = dict(transcript=True, index_base=BASE, amount64=amount64)
    recs, sc = bv.prove_batch_mixed(vals, gams, blind_key=KEY, **wkw)
    recs2, sc2 = bv.prove_batch_mixed(vals, gams, blind_key=KEY2, **wkw)
    recs, sc = list(recs), list(sc)
    recs[OTHER], sc[OTHER] = recs2[OTHER], sc2[OTHER]
    maker = [KEY2 if i == OTHER else KEY for i in range(len(SCAN_MS))]
    chs = [TR._checker_challenges(cname, N, m, recs[i], sc[i]) for i, m in enumerate(SCAN_MS)]
    gamma = [[_gamma_bigint(cname, N, m, sc[i], chs[i], key, BASE + i) for i, m in enumerate(SCAN_MS)] for key in KEYS]
    status, masks = [], []
    for j, key in enumerate(KEYS):
        st = []
        for i, m in enumerate(SCAN_MS):
            if i == DAMAGED:
                st.append(2)
            elif m > 1:
                st.append(3)
            else:
                st.append(0 if maker[i] == key and i != WRONG else 1)
            if maker[i] == key and i != DAMAGED:   # the owner reads the chosen masks
                assert gamma[j][i] == RC.gamma_of(r, gams[i], chs[i][1] if m > 1 else 0)
        status.append(st)
        masks.append([gamma[j][i] if s in (0, 3) else 0 for i, s in enumerate(st)])
    assert status == [[0, 1, 1, 2, 3, 3, 0], [1, 0, 1, 2, 3, 3, 1], [1, 1, 1, 2, 3, 3, 1]]
    assert masks[0][OWN] == gams[OWN][0] and masks[1][OTHER] == gams[OTHER][0] and masks[0][BIG] == gams[BIG][0]
    blk = dict(B=B, bv=bv, raw=b"".join(pr), cm=b"".join(cs), amounts=amounts, status=status, masks=masks, gamma=gamma)
    _blocks[(cname, amount64, version)] = blk
    return blk


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for blk in _blocks.values():
        blk["bv"].close()
    _blocks.clear()


@pytest.mark.parametrize("amount64", (False, True))
@pytest.mark.parametrize("cname", CURVES)
def test_block_of_mixed_ownership(cname, amount64):
    """K = 3 keys over the block of test_scan_from_bytes: the block's key, the key one proof was made under, a key that owns
    nothing.  The exact 3 x 7 status matrix and masks: the chosen gammas under 0, zero under 1 and 2, the big-integer Gamma
    of that (key, proof) under 3, the damaged container 2 under every key.  Without amounts: 3 everywhere but the damaged
    row, Gamma of every pair.  Shuffled with the index as a list: rows follow their proofs."""
    need_gpu()
    blk = _block(cname, amount64, 1)
    bv, raw, cm = blk["bv"], blk["raw"], blk["cm"]
    am = [blk["amounts"]] * len(KEYS)
    st, got = bv.scan_serialized_mixed_keys(raw, cm, SCAN_MS, KEYS, amount64=amount64, index_base=BASE, amounts=am)
    assert st.tolist() == blk["status"] and got == blk["masks"]
    st, got = bv.scan_serialized_mixed_keys(raw, cm, SCAN_MS, KEYS, amount64=amount64,
                                            index=[BASE + i for i in range(len(SCAN_MS))])
    assert st.tolist() == [[2 if i == DAMAGED else 3 for i in range(len(SCAN_MS))]] * len(KEYS)
    assert got == [[0 if i == DAMAGED else g for i, g in enumerate(row)] for row in blk["gamma"]]
    perm = [5, 0, 6, 3, 1, 4, 2]
    pr, cs = TR._split_bytes(blk["B"], bv.arith, raw, cm, SCAN_MS, 1)
    st, got = bv.scan_serialized_mixed_keys(b"".join(pr[j] for j in perm), b"".join(cs[j] for j in perm),
                                            [SCAN_MS[j] for j in perm], KEYS, amount64=amount64,
                                            index=[BASE + j for j in perm], amounts=[[blk["amounts"][j] for j in perm]] * len(KEYS))
    assert st.tolist() == [[row[j] for j in perm] for row in blk["status"]]
    assert got == [[row[j] for j in perm] for row in blk["masks"]]


@pytest.mark.parametrize("cname", CURVES)
def test_agrees_with_the_single_key_call(cname):
    """K = 1, and each key of K = 3: status and masks are scan_serialized_mixed's with that key, word for word -- with
    candidate amounts and without"""
    need_gpu()
    blk = _block(cname, False, 1)
    bv, raw, cm = blk["bv"], blk["raw"], blk["cm"]
    for amounts in (blk["amounts"], None):
        single = [bv.scan_serialized_mixed(raw, cm, SCAN_MS, transcript=True, blind_key=key, index_base=BASE, amounts=amounts)
                  for key in KEYS]
        st, got = bv.scan_serialized_mixed_keys(raw, cm, SCAN_MS, KEYS, index_base=BASE,
                                                amounts=None if amounts is None else [amounts] * len(KEYS))
        assert st.dtype == np.uint32 and st.shape == (len(KEYS), len(SCAN_MS))
        assert st.tolist() == [s.tolist() for s, _ in single] and got == [m for _, m in single]
        for key, (s1, m1) in zip(KEYS, single):
            st, got = bv.scan_serialized_mixed_keys(raw, cm, SCAN_MS, [key], index_base=BASE,
                                                    amounts=None if amounts is None else [amounts])
            assert st.tolist() == [s1.tolist()] and got == [m1]


@pytest.mark.parametrize("n_keys,count", ((1, 1), (3, 7), (5, 67), (64, 1)))
def test_pair_grid_edges(n_keys, count):
    """(8, 1) proofs by the device prover on secp256k1, key j owning the proofs with i mod K == j (each key's proofs made in
    a call of their own, so proof i carries index BASE + i // K): a pair count below one lane group, not a multiple of the
    groups per wave, not a multiple of the confirmation's block.  The whole matrix: 0 and the chosen mask for the owner, 1
    and zero for everybody else."""
    need_gpu()
    cname = "secp256k1"
    r = RC.ORDER[cname]
    B, a, bv = TR._engine(cname, N, 1)
    rng = random.Random(6100 + 100 * n_keys + count)
    keys = [hashlib.sha256(b"grid key %d" % j).digest() for j in range(n_keys)]
    vals = [[rng.randrange(256)] for _ in range(count)]
    gams = [[rng.randrange(r)] for _ in range(count)]
    pr, cs = [None] * count, [None] * count
    for j in range(min(n_keys, count)):
        mine = list(range(j, count, n_keys))
        raw, cm, ms = bv.prove_serialized_mixed([vals[i] for i in mine], [gams[i] for i in mine], blind_key=keys[j],
                                                transcript=True, index_base=BASE)
        p1, c1 = TR._split_bytes(B, a, raw, cm, [1] * len(mine), 1)
        for at, i in enumerate(mine):
            pr[i], cs[i] = p1[at], c1[at]
    st, got = bv.scan_serialized_mixed_keys(b"".join(pr), b"".join(cs), [1] * count, keys,
                                            index=[BASE + i // n_keys for i in range(count)],
                                            amounts=[[v[0] for v in vals]] * n_keys)
    assert st.tolist() == [[0 if i % n_keys == j else 1 for i in range(count)] for j in range(n_keys)]
    assert got == [[gams[i][0] if i % n_keys == j else 0 for i in range(count)] for j in range(n_keys)]
    bv.close()


def test_largest_slot_count():
    """BLS12-381 at the (64, 16) engine shape, m = [16, 1, 16], K = 2: k = 10 is 23 live slots, three strides of a lane
    group.  Gamma of all six pairs from the big-integer formula; for the owner it is gamma_of as well."""
    need_gpu()
    import bulletproofsplus_amd as B
    cname, n = "bls12_381", 64
    r = RC.ORDER[cname]
    a = B.Arith(cname)
    bv = B.BatchVerifier(B.PublicKey.new(a, 64 * 16), 64, 16, window_bits=TR.WB)
    ms = [16, 1, 16]
    vals, gams = TR._inputs(cname, ms, n, 6200)
    raw, cm, got_ms = bv.prove_serialized_mixed(vals, gams, blind_key=KEY, transcript=True, index_base=BASE)
    recs, sc = bv.prove_batch_mixed(vals, gams, transcript=True, blind_key=KEY, index_base=BASE)
    assert got_ms.tolist() == ms
    chs = [TR._checker_challenges(cname, n, m, recs[i], sc[i]) for i, m in enumerate(ms)]
    want = [[_gamma_bigint(cname, n, m, sc[i], chs[i], key, BASE + i) for i, m in enumerate(ms)] for key in (KEY, KEY2)]
    zs = [ch[1] for ch in chs]
    assert want[0] == [RC.gamma_of(r, g, z) for g, z in zip(gams, zs)] and want[0][1] == gams[1][0]
    assert all(x != y for x, y in zip(want[0], want[1]))
    st, got = bv.scan_serialized_mixed_keys(raw, cm, ms, [KEY, KEY2], index_base=BASE)
    assert st.tolist() == [[3, 3, 3]] * 2 and got == want
    bv.close()


@pytest.mark.parametrize("cname", CURVES)
def test_host_twin_at_one_proof_and_the_block_with_and_without_index_and_amounts(cname):
    """bpp_range_scan_serialized_mixed_keys on host pointers at one proof (a single output, an aggregated one) and at the
    block: with the index list and the candidate amounts present, and with both absent (index_base alone: Gamma of every
    pair, nothing confirmed) -- against the block's big-integer statuses and masks"""
    need_gpu()
    blk = _block(cname, False, 1)
    bv, raw, cm = blk["bv"], blk["raw"], blk["cm"]
    pr, cs = TR._split_bytes(blk["B"], bv.arith, raw, cm, SCAN_MS, 1)
    for sel in ([OWN], [4], list(range(len(SCAN_MS)))):
        p_, c_, ms_ = b"".join(pr[j] for j in sel), b"".join(cs[j] for j in sel), [SCAN_MS[j] for j in sel]
        st, got = bv.scan_serialized_mixed_keys(p_, c_, ms_, KEYS, index=[BASE + j for j in sel],
                                                amounts=[[blk["amounts"][j] for j in sel]] * len(KEYS))
        assert st.tolist() == [[row[j] for j in sel] for row in blk["status"]], sel
        assert got == [[row[j] for j in sel] for row in blk["masks"]], sel
        st, got = bv.scan_serialized_mixed_keys(p_, c_, ms_, KEYS, index_base=BASE + sel[0])
        assert st.tolist() == [[2 if j == DAMAGED else 3 for j in sel]] * len(KEYS), sel
        assert got == [[0 if j == DAMAGED else row[j] for j in sel] for row in blk["gamma"]], sel


def test_version_2_containers():
    need_gpu()
    blk = _block("bls12_381", True, 2)
    st, got = blk["bv"].scan_serialized_mixed_keys(blk["raw"], blk["cm"], SCAN_MS, KEYS, uncompressed=True, amount64=True,
                                                   index_base=BASE, amounts=[blk["amounts"]] * len(KEYS))
    assert st.tolist() == blk["status"] and got == blk["masks"]


def test_errors_that_need_an_engine():
    """a workspace smaller than the layout: BPP_E_ARG, nothing enqueued, nothing written; the size does not depend on the
    number of keys, is 0 for an m_i above the engine's m, and the device call fills key-major outputs"""
    torch = need_gpu()
    B, a, bv = TR._engine("secp256k1")
    ms = [1, 2, 4, 1]
    wsb = bv.scan_keys_workspace_bytes(ms, 3)
    assert wsb > 0 and wsb == bv.scan_keys_workspace_bytes(ms, 1) and bv.scan_keys_workspace_bytes([1, 8], 3) == 0
    d = torch.full((4096,), 0x5a, dtype=torch.uint8, device="cuda:0")
    p = d.data_ptr()
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(B.BppError) as ei:
        bv.scan_serialized_mixed_keys_device(p, p, ms, p, 3, p, p, d_ws.data_ptr(), wsb - 1)
    assert ei.value.code == -1 and "workspace too small" in str(ei.value)
    with pytest.raises(B.BppError) as ei:
        bv.scan_serialized_mixed_keys_device(p, p, [8, 1], p, 3, p, p, d_ws.data_ptr(), wsb)
    assert ei.value.code == -1 and "m_of[0]" in str(ei.value)
    torch.cuda.synchronize()
    assert d.cpu().tolist() == [0x5a] * 4096
    bv.close()
