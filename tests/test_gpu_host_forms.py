"""-m gpu: the host forms side by side.  Every entry that takes host pointers is its device entry between copies
(csrc/staging.hpp), so what can go wrong in all of them alike is a size and the rule for an absent buffer.

 * count = 0 pins only the ENTRIES' early return (no host form's body runs then): every one answers 0 and leaves
   guard-filled outputs alone, with its optional pointers null and with them set; the two find forms answer their counts,
   bpp_msm_pippenger the empty sum;
 * the five verify twins at count = 1 and on a block of at most 15 cases of the adversarial corpus, against the
   definition's verdicts (verdict_corpus: the C oracle, pyref on edwards25519), one shape (the twins over mixed m_i:
   test_gpu_prove_mixed.py);
 * bpp_range_prove_batch with and without out_V, bpp_range_prove_batch_mixed with and without out_challenges, at count = 1
   and on a small block, against the oracle's proofs.
Each other family runs its host forms at one item and at a small block, optional inputs absent and present, in its own
file (test_gpu_recover.py, test_gpu_recover_keys.py, test_gpu_find.py, test_gpu_find_tags.py, test_gpu_prove_mixed.py,
test_gpu_amount64.py, test_gpu_wip.py, test_gpu_container.py, test_codec.py)."""

import ctypes

import numpy as np
import pytest

import oracle as O
import pyref as P
import verdict_corpus as VC
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

GUARD = 0xA7


def _engine(cp, window_bits=5):
    import bulletproofsplus_amd as B
    a = B.Arith(cp.cname)
    pk = B.PublicKey.from_points(a, cp.gh, cp.G, cp.H)
    return B, a, B.BatchVerifier(pk, cp.n, cp.m, window_bits=window_bits)


def _guard(nbytes):
    return np.full(nbytes, GUARD, dtype=np.uint8)


def _p(x):
    return None if x is None else ctypes.c_void_p(x.ctypes.data)


def test_count_zero_touches_nothing():
    need_gpu()
    from bulletproofsplus_amd import _lib
    cp = VC.corpus("bls12_381", 8, 2)
    B, a, bv = _engine(cp)
    L, h, ah = _lib.lib(), bv.handle, a.handle
    src = _guard(4096)            # every input: readable, never read
    outs = [_guard(4096) for _ in range(4)]
    o = [_p(x) for x in outs]
    s, key = _p(src), bytes(range(32))
    m_of = np.array([2], dtype=np.uint32)
    for present in (False, True):
        i = s if present else None          # an optional input: index, blinding, amounts, challenges, transcript
        x = (lambda k: o[k]) if present else (lambda k: None)   # an optional output
        calls = {
            "verify_batch": lambda: L.bpp_range_verify_batch(h, s, s, 0, o[0]),
            "verify_batch_mixed": lambda: L.bpp_range_verify_batch_mixed(h, s, s, _p(m_of), 0, o[0]),
            "verify_batch_compressed": lambda: L.bpp_range_verify_batch_compressed(h, s, s, 0, o[0]),
            "verify_batch_serialized": lambda: L.bpp_range_verify_batch_serialized(h, s, s, 0, 0, o[0]),
            "verify_batch_serialized_mixed": lambda: L.bpp_range_verify_batch_serialized_mixed(h, s, s, _p(m_of), 0, 0, o[0]),
            "prove_batch": lambda: L.bpp_range_prove_batch(h, s, s, 0, o[0], o[1], x(2)),
            "prove_batch_fs": lambda: L.bpp_range_prove_batch_fs(h, s, s, 0, key, 0, o[0], o[1], x(2)),
            "prove_batch_mixed": lambda: L.bpp_range_prove_batch_mixed(h, s, s, _p(m_of), 0, 1, key if present else None, 0, o[0],
                                                                       o[1], x(2)),
            "prove_batch_serialized_mixed": lambda: L.bpp_range_prove_batch_serialized_mixed(h, s, s, _p(m_of), 0, 1,
                                                                                             key if present else None, 0, o[0], o[1]),
            "commit_batch": lambda: L.bpp_commit_batch(h, s, s, 0, 0, o[0]),
            "recover_masks_mixed": lambda: L.bpp_range_recover_masks_mixed(h, s, _p(m_of), 0, i, key if present else None, 0, i,
                                                                           None, o[0]),
            "scan_serialized_mixed": lambda: L.bpp_range_scan_serialized_mixed(h, s, s, _p(m_of), 0, 1, key if present else None, 0,
                                                                               i, None, i, o[0], o[1]),
            "scan_serialized_mixed_keys": lambda: L.bpp_range_scan_serialized_mixed_keys(h, s, s, _p(m_of), 0, 1, s, 1, 0, i, i,
                                                                                         o[0], o[1]),
            "amounts_seal": lambda: L.bpp_amounts_seal(ah, key, 0, i, s, 0, o[0]),
            "view_tags": lambda: L.bpp_view_tags(ah, key, 0, i, 0, o[0]),
            "wip_prove_batch": lambda: L.bpp_wip_prove_batch(h, s, s, s, s, 0, 0, 1 if present else 0, i, None, 0, i, o[0], o[1], x(2)),
            "wip_verify_batch": lambda: L.bpp_wip_verify_batch(h, s, s, s, s, 0, 0, 1 if present else 0, i, None, o[0], x(1), x(2)),
            "points_compress": lambda: L.bpp_points_compress(ah, s, 0, o[0]),
            "points_decompress": lambda: L.bpp_points_decompress(ah, s, 0, o[0], o[1]),
            "proofs_encode": lambda: L.bpp_proofs_encode_version(ah, 8, 2, 1, s, s, 0, o[0]),
            "proofs_decode": lambda: L.bpp_proofs_decode(ah, 8, 2, s, 0, o[0], o[1], o[2]),
        }
        for name, call in calls.items():
            assert call() == 0, (name, present, L.bpp_last_error())
            assert all((g == GUARD).all() for g in outs), (name, present)
    assert (src == GUARD).all()
    # the find forms answer their counts: no proof, no hit, no candidate -- and write nothing else
    n_hits, n_cand = np.full(1, 7, dtype=np.uint32), np.full(1, 7, dtype=np.uint32)
    assert L.bpp_range_verify_find_serialized_mixed_keys(h, s, s, _p(m_of), 0, 1, s, 1, 0, None, s, o[0], o[1], 8, _p(n_hits)) == 0
    assert n_hits[0] == 0
    n_hits[0] = 7
    assert L.bpp_range_verify_find_tagged_serialized_mixed_keys(h, s, s, _p(m_of), 0, 1, s, 1, 0, None, s, o[0], o[1], 8,
                                                                _p(n_hits), s, _p(n_cand)) == 0
    assert n_hits[0] == 0 and n_cand[0] == 0
    # ... and the empty MulVec is the point at infinity
    out = np.full(a.PW, 7, dtype=np.uint64)
    assert L.bpp_msm_pippenger(ah, s, s, 0, 0, _p(out)) == 0
    assert out[:-1].tolist() == [0] * (a.PW - 1) and out[-1] == 1
    assert all((x == GUARD).all() for x in outs)
    bv.close()


@pytest.mark.parametrize("cname", ["bls12_381", "secp256k1", "ed25519"])
def test_verify_twins_at_count_one_and_on_a_small_block(cname):
    need_gpu()
    cp = VC.corpus(cname, 8, 2)
    B, a, bv = _engine(cp)
    ms = lambda k: [cp.m] * k
    # wire records: every case whose record has the engine's length and whose verdict the raw pass defines (without the
    # subgroup check a BLS12-381 point outside G1 is the caller's fault: test_gpu_verdict_parity.py, _raw_expect)
    wire = [c for c in cp.cases if c.k_ok and not (cname == "bls12_381" and c.shifted)]
    want_w = [c.expect for c in wire]
    # encodings: every case that has one, with the decoder's status
    ser = [c for c in cp.cases if c.status is not None]
    want_s = [c.status for c in ser]
    # the corpus has all three answers (on secp256k1, of cofactor 1, no encoding of it earns a FormatError)
    assert {0, 1} == set(want_w) and set(want_s) == ({0, 1} if cname == "secp256k1" else {0, 1, 2})
    cb = B.compressed_bytes(a)
    recs_c = [np.frombuffer(b"".join(P.compress_point(cp.curve, Pt) for Pt in
                                     O.wire_to_points(cp.cid, VC.canonical_inf(cp, np.concatenate([c.pts, c.V])))),
                            np.uint8).reshape(-1, cb) for c in ser]
    enc = [VC.encode_case(cp, c, 1) for c in ser]
    proofs = [np.frombuffer(b, np.uint8) for b, _ in enc]
    comms = [np.frombuffer(m, np.uint8) for _, m in enc]

    def pick(want, count):
        """`count` indices: a rejected case alone; else accepted and rejected ones mixed, a rejected one first and last"""
        bad = [i for i, w in enumerate(want) if w]
        if count == 1:
            return [bad[0]]
        idx = [i % len(want) for i in range(count)]
        idx[0], idx[-1] = bad[0], bad[-1]
        return idx

    for count in (1, min(15, len(wire))):
        iw = pick(want_w, count)
        recs = np.stack([np.concatenate([wire[i].pts, wire[i].V]) for i in iw])
        scs = np.stack([wire[i].sc for i in iw])
        assert bv.verify_wire(recs, scs).tolist() == [want_w[i] for i in iw], count
        assert bv.verify_wire_mixed(list(recs), scs, ms(count)).tolist() == [want_w[i] for i in iw], count
    for count in (1, min(15, len(ser))):
        i_s = pick(want_s, count)
        exp = [want_s[i] for i in i_s]
        scs = np.stack([ser[i].sc for i in i_s])
        assert bv.verify_compressed(np.stack([recs_c[i] for i in i_s]), scs).tolist() == exp, count
        pr, cm = np.stack([proofs[i] for i in i_s]), np.stack([comms[i] for i in i_s])
        assert bv.verify_serialized(pr, cm).tolist() == exp, count
        assert bv.verify_serialized_mixed(pr.reshape(-1), cm.reshape(-1), ms(count)).tolist() == exp, count
    bv.close()


@pytest.mark.parametrize("cname", ["bls12_381", "secp256k1"])
def test_prove_forms_with_and_without_their_optional_outputs(cname):
    need_gpu()
    from bulletproofsplus_amd import _lib
    import bulletproofsplus_amd as B
    n, m, cid = 8, 2, VC.CID[cname]
    a = B.Arith.init(cid)
    opk = O.PublicKey(cid, n * m)
    eng = B.BatchVerifier(B.PublicKey.from_points(a, opk.gh, opk.G, opk.H), n, m, window_bits=5)
    L, PW, k = _lib.lib(), a.PW, 4
    r = P.CURVES[cname]["r"]
    for count in (1, 5):
        vals = [[(37 * i + 11 * j + 5) % (1 << n) for j in range(m)] for i in range(count)]
        gams = [[(i * 1000003 + j * 7919 + 1) % r for j in range(m)] for i in range(count)]
        want = [O.range_prove(opk, n, v, g) for v, g in zip(vals, gams)]
        v_arr = np.array(vals, dtype=np.uint64)
        g_arr = O.scalars_to_wire([g for row in gams for g in row])
        m_of = np.full(count, m, dtype=np.uint32)
        for optional in (False, True):
            pts, sc = np.zeros((count, 3 + 2 * k, PW), dtype=np.uint64), np.zeros((count, 3, 4), dtype=np.uint64)
            V = np.zeros((count, m, PW), dtype=np.uint64) if optional else None
            assert L.bpp_range_prove_batch(eng.handle, _p(v_arr), _p(g_arr), count, _p(pts), _p(sc), _p(V)) == 0, L.bpp_last_error()
            for i, (opts, osc, oV) in enumerate(want):
                assert np.array_equal(pts[i], opts) and np.array_equal(sc[i], osc), (count, optional, i)
                assert V is None or np.array_equal(V[i], oV), (count, i)
            # the mixed form on the same block: literal mode, so the proofs are the oracle's again and the challenges the literals
            pts2, sc2 = np.zeros((count, 3 + 2 * k + m, PW), dtype=np.uint64), np.zeros_like(sc)   # records: V included
            ch = np.zeros((count, 3 + k, 4), dtype=np.uint64) if optional else None
            assert L.bpp_range_prove_batch_mixed(eng.handle, _p(v_arr), _p(g_arr), _p(m_of), count, 0, None, 0, _p(pts2), _p(sc2),
                                                 _p(ch)) == 0, L.bpp_last_error()
            assert np.array_equal(pts2[:, :3 + 2 * k], pts) and np.array_equal(sc2, sc), (count, optional)
            assert np.array_equal(pts2[:, 3 + 2 * k:], np.stack([oV for _, _, oV in want])), (count, optional)
            if optional:
                assert [O.wire_to_scalars(c) for c in ch] == [[12, 23, 99] + [7] * k] * count
    eng.close()
