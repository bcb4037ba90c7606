"""-m gpu: the three verify-and-find calls -- rewinding, rewinding with view tags, per output -- are one host engine under
three modes (csrc/find.hpp: FindEngine; csrc/outputs.hpp supplies the per-output class step).  ONE block goes through all
three, so that what the engine does once is seen to be the same thing each time: the verdicts, the host twin against the
device entry, the max_hits rule, the call without keys.

Expected values never come from the library.  Every single output is proved under its owner's key with the mask
output_cases.mask gives it at place 0, so the owner finds it by rewinding AND by its derived mask; pads, tags and masks are
hashlib's; the verdicts are what the test did to the containers, and verify_serialized_mixed's on the same bytes.  The
device entries are driven by the helpers of the three calls' own test files."""

import hashlib

import numpy as np
import pytest

import find_cases as FC
import output_cases as OC
import recover_cases as RC
import tag_cases as TC
import test_gpu_find as TF
import test_gpu_find_tags as TG
import test_gpu_outputs as TO
import test_gpu_recover as TR
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

CURVES, N, BASE, GUARD = TR.CURVES, TR.N, TR.BASE, TF.GUARD
K0, K1, K2 = (hashlib.sha256(b"find engine: scanning key %d" % q).digest() for q in range(3))
FOREIGN = hashlib.sha256(b"find engine: a key nobody scans with").digest()
SENDER = hashlib.sha256(b"find engine: the sender's blinding key").digest()
KEYS = [K0, K1, K2]

MS = [1, 2, 1, 4, 1, 1, 2]
FIRST = [sum(MS[:i]) for i in range(len(MS))]
N_OUT = sum(MS)
PROOF_OF = [i for i, m in enumerate(MS) for _ in range(m)]
PLACE_OF = [j for m in MS for j in range(m)]
INDEX = [BASE + i for i in range(len(MS))]
DAMAGED, SWAPPED = 1, 6        # a flipped header byte the decoder rejects; a commitment that is another proof's
VERDICT = [0, 2, 0, 0, 0, 0, 1]
OWNER = [K0,   K1, K0,   K1,   K0, K1, FOREIGN, K2,   K0,   K2,   K2, K1]
assert len(OWNER) == N_OUT and [OWNER[FIRST[i]] for i in (0, 2, 4, 5)] == [K0, K1, K0, K2]


def _block(cname):
    """-> dict(bv, raw, cm, amounts, masks (per output), psealed, ptags (per proof, the rewinding calls'), osealed, otags
    (per output), hits {mode: [(key_no, unit, amount, mask)]}, cands {mode: count})"""
    r = RC.ORDER[cname]
    B, a, bv = TR._engine(cname)
    amounts = [17 + 13 * o for o in range(N_OUT)]
    masks = [OC.mask(OWNER[o], INDEX[PROOF_OF[o]], PLACE_OF[o], r) for o in range(N_OUT)]
    pr, cs = [], []
    for i, m in enumerate(MS):   # a single output under its owner's key, so that rewinding finds the mask it was given
        o = FIRST[i]
        raw, cm, _ = bv.prove_serialized_mixed([amounts[o:o + m]], [masks[o:o + m]], transcript=True,
                                               blind_key=OWNER[o] if m == 1 else SENDER, index_base=INDEX[i])
        pr.append(bytes(raw))
        cs.append(bytes(cm))
    bad = bytearray(pr[DAMAGED])
    bad[7] ^= 3   # the header's m
    pr[DAMAGED] = bytes(bad)
    pb = B.compressed_bytes(a)
    assert cs[DAMAGED][:pb] != cs[SWAPPED][:pb]
    cs[SWAPPED] = cs[DAMAGED][:pb] + cs[SWAPPED][pb:]   # a valid point, and not the one the proof is about
    osealed = [amounts[o] ^ OC.pad(OWNER[o], INDEX[PROOF_OF[o]], PLACE_OF[o]) for o in range(N_OUT)]
    otags = [OC.tag(OWNER[o], INDEX[PROOF_OF[o]], PLACE_OF[o]) for o in range(N_OUT)]
    psealed, ptags = [osealed[FIRST[i]] for i in range(len(MS))], [otags[FIRST[i]] for i in range(len(MS))]
    singles = [i for i, m in enumerate(MS) if m == 1]
    assert [psealed[i] for i in singles] == [amounts[FIRST[i]] ^ FC.pad(OWNER[FIRST[i]], INDEX[i]) for i in singles]
    assert [ptags[i] for i in singles] == [TC.tag(OWNER[FIRST[i]], INDEX[i]) for i in singles]
    rewound = [(q, i, amounts[FIRST[i]], masks[FIRST[i]]) for q, k in enumerate(KEYS) for i in singles if OWNER[FIRST[i]] == k]
    listed = [(q, o, amounts[o], masks[o]) for q, k in enumerate(KEYS) for o in range(N_OUT)
              if OWNER[o] == k and VERDICT[PROOF_OF[o]] == 0]
    assert len(rewound) == 4 and len(listed) == 7
    eligible = [m == 1 and v == 0 for m, v in zip(MS, VERDICT)]
    cands = {"tagged": len(TC.candidates(KEYS, INDEX, ptags, eligible)),
             "outputs": len(TO._candidates(KEYS, INDEX, MS, otags, VERDICT))}
    return dict(bv=bv, raw=b"".join(pr), cm=b"".join(cs), psealed=psealed, ptags=ptags, osealed=osealed, otags=otags,
                hits={"untagged": rewound, "tagged": rewound, "outputs": listed}, cands=cands)


def _host(blk, mode, keys, max_hits=None):
    """the host form of a mode -> (ok, hits, n_hits, n_candidates or None)"""
    bv, raw, cm = blk["bv"], blk["raw"], blk["cm"]
    if mode == "outputs":
        ok, hits, found, n_cand = bv.verify_find_outputs_serialized_mixed_keys(raw, cm, MS, keys, blk["osealed"], blk["otags"],
                                                                               index_base=BASE, max_hits=max_hits)
        return ok.tolist(), hits, found, n_cand
    out = bv.verify_find_serialized_mixed_keys(raw, cm, MS, keys, amounts=blk["psealed"], sealed=True, index_base=BASE,
                                               max_hits=max_hits, tags=blk["ptags"] if mode == "tagged" else None)
    return (out[0].tolist(),) + tuple(out[1:]) + ((None,) if mode == "untagged" else ())


def _device(torch, blk, mode, max_hits):
    """the device entry of a mode over guard words -> (ok, all words of d_hits, n_hits, n_candidates or None)"""
    bv, raw, cm = blk["bv"], blk["raw"], blk["cm"]
    if mode == "outputs":
        return TO._find_device(torch, bv, raw, cm, MS, KEYS, blk["osealed"], blk["otags"], INDEX, max_hits)[:4]
    if mode == "tagged":
        return TG._find_device(torch, bv, raw, cm, MS, KEYS, blk["psealed"], INDEX, blk["ptags"], max_hits, True)
    return TF._find_device(torch, bv, raw, cm, MS, KEYS, blk["psealed"], INDEX, max_hits, True) + (None,)


def _device_without_keys(torch, blk, mode):
    """the device entry of a mode with no key, and no buffer that only keys need -> (ok, [n_hits, guard, n_candidates, guard])"""
    bv = blk["bv"]
    d_p = torch.frombuffer(bytearray(blk["raw"]), dtype=torch.uint8).to("cuda:0")
    d_c = torch.frombuffer(bytearray(blk["cm"]), dtype=torch.uint8).to("cuda:0")
    d_ok = TR._dev(torch, np.full(len(MS), GUARD, dtype=np.uint32))
    d_n = TR._dev(torch, np.full(4, GUARD, dtype=np.uint32))
    st = torch.cuda.current_stream().cuda_stream
    if mode == "outputs":
        wsb = bv.verify_find_outputs_workspace_bytes(MS, 0)
        d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
        bv.verify_find_outputs_serialized_mixed_keys_device(d_p.data_ptr(), d_c.data_ptr(), MS, 0, 0, 0, 0, d_ok.data_ptr(), 0, 4,
                                                            d_n.data_ptr(), d_ws.data_ptr(), wsb, st, index_base=BASE,
                                                            d_n_candidates=d_n.data_ptr() + 8)
    else:
        tagged = mode == "tagged"
        wsb = (bv.verify_find_tagged_workspace_bytes if tagged else bv.verify_find_workspace_bytes)(MS, 0)
        d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
        d_t = TR._dev(torch, np.array(blk["ptags"], dtype=np.uint8))   # what selects the tagged entry; unread without keys
        bv.verify_find_serialized_mixed_keys_device(d_p.data_ptr(), d_c.data_ptr(), MS, 0, 0, 0, d_ok.data_ptr(), 0, 4,
                                                    d_n.data_ptr(), d_ws.data_ptr(), wsb, st, sealed=True, index_base=BASE,
                                                    d_tags=d_t.data_ptr() if tagged else 0,
                                                    d_n_candidates=d_n.data_ptr() + 8 if tagged else 0)
    torch.cuda.synchronize()
    return d_ok.cpu().numpy().view(np.uint32).tolist(), d_n.cpu().numpy().view(np.uint32).tolist()


@pytest.mark.parametrize("cname", CURVES)
def test_one_block_through_the_three_modes(cname):
    """m_of = [1, 2, 1, 4, 1, 1, 2] on the (8, 4) engine under three keys, a fourth owning an output; container 1 damaged,
    container 6 with a foreign commitment.  The three calls write the same verdicts, verify_serialized_mixed's; per call
    the host twin and the device entry agree word for word; max_hits = n_hits - 1 reports all hits and writes that many
    records less one; without keys every verdict is written and the counts are zero."""
    torch = need_gpu()
    blk = _block(cname)
    bv = blk["bv"]
    plain = bv.verify_serialized_mixed(blk["raw"], blk["cm"], MS, transcript=True).tolist()
    assert plain == VERDICT
    for mode in ("untagged", "tagged", "outputs"):
        want, n_cand = blk["hits"][mode], blk["cands"].get(mode)
        n_hits = len(want)
        assert n_hits >= 4 and want == sorted(want)
        host = _host(blk, mode, KEYS)
        assert host == (plain, want, n_hits, n_cand), mode
        ok, words, found, cands = _device(torch, blk, mode, n_hits)
        assert (ok, found, cands) == (plain, n_hits, n_cand), mode
        assert words[:n_hits].tolist() == TF._records(host[1]) and (words[n_hits:] == GUARD).all(), mode
        # one record short: the count is of the hits there are, the records are the first ones
        assert _host(blk, mode, KEYS, max_hits=n_hits - 1) == (plain, want[:n_hits - 1], n_hits, n_cand), mode
        ok, words, found, cands = _device(torch, blk, mode, n_hits - 1)
        assert (ok, found, cands) == (plain, n_hits, n_cand), mode
        assert words[:n_hits - 1].tolist() == TF._records(want[:n_hits - 1]) and (words[n_hits - 1:] == GUARD).all(), mode
        # no key: a verification all the same
        assert _host(blk, mode, []) == (plain, [], 0, None if mode == "untagged" else 0), mode
        ok, counts = _device_without_keys(torch, blk, mode)
        assert ok == plain and counts == [0, GUARD, GUARD if mode == "untagged" else 0, GUARD], mode
    bv.close()
