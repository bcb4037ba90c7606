"""-m gpu: the WIP seam -- WeightedInnerProductProof::{prove, verify} as batched entry points of an engine
(bpp_wip_prove_batch_device, bpp_wip_verify_batch_device and their host forms; include/bpp_amd.h).

The prover is pinned bit for bit against pyref's restatement of wip.rs:36-227 (literal mode, under a caller-owned
transcript, with blinding, and across a chunk of the prover's workspace) and against the engine's own range prover; the
verifier against bpp_verifier_run on range statements (m = 1: scalars and result identical; m > 1: verdicts), against pyref's verify_mulvec scalar list and the
oracle's MulVec of it on a sweep of geometries, and for the subgroup check, the usage errors and y = 0."""

import hashlib
import random

import numpy as np
import pytest

import oracle as O
import pyref as P
import verdict_corpus as VC
import wip_cases as W
from gpu_util import need_gpu, run_verifier_device

pytestmark = pytest.mark.gpu

SENT = 0x5A


class Ctx:
    """one curve, one key of `length` generators (the oracle's PublicKey::new), one engine (n, m) with n m = length"""

    def __init__(self, cname, n, m, wb, shadow_pk=False):
        import bulletproofsplus_amd as B
        self.B, self.cname, self.cid = B, cname, VC.CID[cname]
        self.cp = VC.Corpus(cname, n, m, False)
        self.r, self.length = self.cp.r, n * m
        self.k = self.length.bit_length() - 1
        self.a = B.Arith.init(cname)
        self.PW = self.a.PW
        self.bv = B.BatchVerifier(B.PublicKey.from_points(self.a, self.cp.gh, self.cp.G, self.cp.H), n, m, window_bits=wb)
        # pyref's key over the real group (the definition), or over the shadow group when only scalars are wanted
        self.grp = P.ShadowGroup(self.r) if shadow_pk else self.cp.grp
        self.pk = self.cp.ppk if (cname == "ed25519" and not shadow_pk) else P.PublicKey(self.grp, self.length)

    def wire(self, pts):
        return O.points_to_wire(self.cid, list(pts))

    def msm(self, scalars, points):
        """the definition's MulVec: the C oracle, or pyref's Edwards group"""
        if self.cname == "ed25519":
            return self.cp.grp.msm([s % self.r for s in scalars], points)
        return O.wire_to_point(self.cid, O.msm(self.cid, O.scalars_to_wire([s % self.r for s in scalars]), self.wire(points)))


def _dev(torch, x):
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.uint8).reshape(-1)).to(torch.device("cuda:0"))


def _rows_wire(rows):
    """scalars (a list, or a list of rows) in wire form; an array is taken to be in wire form already"""
    if isinstance(rows, np.ndarray):
        return rows
    rows = list(rows)
    return O.scalars_to_wire([x for row in rows for x in row] if rows and isinstance(rows[0], (list, tuple)) else rows)


def _prove_device(torch, cx, a, b, y, gamma, nv, transcript=None, blind_key=None, index_base=0, blinding=None):
    """bpp_wip_prove_batch_device into sentinel-filled buffers -> (records (count, 3+2k+nv, PW), scalars, challenges)"""
    bv, count = cx.bv, len(a)
    npts = bv.wip_points_per_proof(nv)
    d_a, d_b = _dev(torch, _rows_wire(a)), _dev(torch, _rows_wire(b))
    d_y, d_g = _dev(torch, _rows_wire(y)), _dev(torch, _rows_wire(gamma))
    d_p = torch.full((count * npts * cx.PW * 8,), SENT, dtype=torch.uint8, device="cuda:0")
    d_s = torch.full((count * 96,), SENT, dtype=torch.uint8, device="cuda:0")
    d_c = torch.full((count * (1 + cx.k) * 32,), SENT, dtype=torch.uint8, device="cuda:0")
    d_t = _dev(torch, np.frombuffer(b"".join(transcript), dtype=np.uint8).copy()) if transcript is not None else None
    d_bl = _dev(torch, _rows_wire(blinding)) if blinding is not None else None
    wsb = bv.wip_prover_workspace_bytes(count)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    bv.wip_prove_device(d_a.data_ptr(), d_b.data_ptr(), d_y.data_ptr(), d_g.data_ptr(), count, nv, d_p.data_ptr(),
                        d_s.data_ptr(), d_ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream,
                        transcript=transcript is not None, d_transcript=d_t.data_ptr() if d_t is not None else 0,
                        blind_key=blind_key, index_base=index_base, d_blinding=d_bl.data_ptr() if d_bl is not None else 0,
                        d_out_challenges=d_c.data_ptr())
    torch.cuda.synchronize()
    return (d_p.cpu().numpy().view(np.uint64).reshape(count, npts, cx.PW),
            d_s.cpu().numpy().view(np.uint64).reshape(count, 3, 4), d_c.cpu().numpy().view(np.uint64).reshape(count, 1 + cx.k, 4))


def _verify_device(torch, cx, rec, sc, y, stm, nv, transcript=None, challenges=None, wsb=None, flags_transcript=None):
    """bpp_wip_verify_batch_device -> (ok, out scalars (count, N, 4), out result (count, PW)); d_ok starts as 7"""
    bv, count = cx.bv, rec.shape[0]
    N = 2 * cx.length + 2 * cx.k + 5 + nv
    d_p, d_s = _dev(torch, rec), _dev(torch, sc)
    d_y = _dev(torch, O.scalars_to_wire(list(y)))
    d_m = _dev(torch, O.scalars_to_wire([x for row in stm for x in row]))
    d_ok = torch.full((count,), 7, dtype=torch.int32, device="cuda:0")
    d_os = torch.zeros((count, N, 4), dtype=torch.int64, device="cuda:0")
    d_or = torch.zeros((count, cx.PW), dtype=torch.int64, device="cuda:0")
    d_t = _dev(torch, np.frombuffer(b"".join(transcript), dtype=np.uint8).copy()) if transcript is not None else None
    d_c = _dev(torch, challenges) if challenges is not None else None
    full = bv.wip_verifier_workspace_bytes(count, nv)
    wsb = full if wsb is None else wsb
    d_ws = torch.empty(max(full, 256), dtype=torch.uint8, device="cuda:0")
    use_tr = (transcript is not None) if flags_transcript is None else flags_transcript
    try:
        bv.wip_verify_device(d_p.data_ptr(), d_s.data_ptr(), d_y.data_ptr(), d_m.data_ptr(), nv, count, d_ok.data_ptr(),
                             d_ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream, transcript=use_tr,
                             d_transcript=d_t.data_ptr() if d_t is not None else 0,
                             d_challenges=d_c.data_ptr() if d_c is not None else 0, d_out_scalars=d_os.data_ptr(),
                             d_out_result=d_or.data_ptr())
    finally:
        torch.cuda.synchronize()
    return d_ok.cpu().numpy().astype(np.uint32), d_os.cpu().numpy().view(np.uint64), d_or.cpu().numpy().view(np.uint64)


# ---- 1. the prover against the restatement, literal mode ----------------------------------------------------------
@pytest.mark.parametrize("cname,n,m", [("bls12_381", 8, 1), ("secp256k1", 8, 2), ("ed25519", 8, 1)])
def test_prover_matches_the_restatement(cname, n, m):
    torch = need_gpu()
    cx = Ctx(cname, n, m, 5)
    nv = 2
    cases = [W.random_case(cx.pk, 0, 11), W.random_case(cx.pk, 0, 12, zero_ends=True), W.random_case(cx.pk, 0, 13, over_r=True)]
    rec, sc, ch = _prove_device(torch, cx, [c.a for c in cases], [c.b for c in cases], [c.y for c in cases],
                                [c.gamma for c in cases], nv)
    k = cx.k
    sent = np.frombuffer(bytes([SENT]) * 8, dtype=np.uint64)[0]
    for i, c in enumerate(cases):
        pf = c.prove()
        exp = [pf.A, pf.B] + list(pf.L_vec) + list(pf.R_vec)
        assert O.wire_to_points(cx.cid, rec[i, 1:3 + 2 * k]) == exp, i
        assert np.array_equal(rec[i, 1:3 + 2 * k], cx.wire(exp)), i
        assert O.wire_to_scalars(sc[i]) == [pf.r_prime, pf.s_prime, pf.d_prime], i
        assert (rec[i, 0] == sent).all() and (rec[i, 3 + 2 * k:] == sent).all(), i      # A' and V are the caller's
        assert O.wire_to_scalars(ch[i]) == [99] + [7] * k


# ---- 2. the seam reproduces the range prover ---------------------------------------------------------------------
def test_seam_reproduces_the_range_prover():
    need_gpu()
    n, m = 8, 2
    cx = Ctx("bls12_381", n, m, 5, shadow_pk=True)
    vals = [[200, 5], [0, 255], [1, 2], [77, 130], [255, 255]]
    gams = [[3 + i, 7 * i + 1] for i in range(5)]
    cases = [W.range_case(cx.pk, n, v, g)[0] for v, g in zip(vals, gams)]     # scalars only: the shadow group is enough
    pts, sc, _ = cx.bv.prove_batch(vals, gams)
    rec, wsc, _ = cx.bv.wip_prove_batch([c.a for c in cases], [c.b for c in cases], [c.y for c in cases],
                                        [c.gamma for c in cases])
    assert np.array_equal(rec[:, 1:], pts[:, 1:])
    assert np.array_equal(wsc, sc)
    assert not rec[:, 0].any()


# ---- 3. under a transcript the caller owns ---------------------------------------------------------------------------
def _fs(cx, state):
    fs = P.FsTranscript(cx.cp.curve, cx.cid, cx.length, 1, cx.pk)
    fs.st = state
    return fs


def _pyref_fs_prove(cx, case, state):
    """pyref's prover continuing the transcript `state`, and the challenges [e, e_1..e_k] it drew"""
    P.Transcript.run = _fs(cx, state)
    try:
        pf = case.prove()
    finally:
        P.Transcript.run = None
    fs = _fs(cx, state)
    fs.wip_start(cx.length)
    es = [fs.round(L, R) for L, R in zip(pf.L_vec, pf.R_vec)]
    return pf, [fs.final(pf.A, pf.B)] + es


def test_transcript_continues_the_callers_state():
    torch = need_gpu()
    cx = Ctx("secp256k1", 8, 1, 5)
    nv = 1
    cases = [W.random_case(cx.pk, nv, 30 + i) for i in range(3)]
    states = [hashlib.sha256(b"caller transcript %d" % i).digest() for i in range(3)]
    rec, sc, ch = _prove_device(torch, cx, [c.a for c in cases], [c.b for c in cases], [c.y for c in cases],
                                [c.gamma for c in cases], nv, transcript=states)
    k = cx.k
    for i, c in enumerate(cases):
        pf, es = _pyref_fs_prove(cx, c, states[i])
        assert np.array_equal(rec[i, 1:3 + 2 * k], cx.wire([pf.A, pf.B] + list(pf.L_vec) + list(pf.R_vec))), i
        assert O.wire_to_scalars(sc[i]) == [pf.r_prime, pf.s_prime, pf.d_prime], i
        assert O.wire_to_scalars(ch[i]) == es, i
        rec[i, 0] = cx.wire([c.A_prime])[0]
        rec[i, 3 + 2 * k:] = cx.wire(c.V)
    y, stm = [c.y for c in cases], [c.statement() for c in cases]
    ok, _, _ = _verify_device(torch, cx, rec, sc, y, stm, nv, transcript=states)
    assert ok.tolist() == [0, 0, 0]
    flipped = list(states)
    flipped[1] = bytes([states[1][0] ^ 1]) + states[1][1:]
    ok, _, _ = _verify_device(torch, cx, rec, sc, y, stm, nv, transcript=flipped)
    assert ok.tolist() == [0, 1, 0]
    ok, _, _ = _verify_device(torch, cx, rec, sc, y, stm, nv, challenges=ch)      # a transcript of the caller's own
    assert ok.tolist() == [0, 0, 0]
    ok, _, _ = _verify_device(torch, cx, rec, sc, y, stm, nv)                     # the literals are not these challenges
    assert ok.tolist() == [1, 1, 1]


# ---- 3b. the host forms, with every optional buffer absent and with every one present ----------------------------------
@pytest.mark.parametrize("count", [1, 3])
def test_host_forms_with_and_without_the_optional_buffers(count):
    """bpp_wip_prove_batch / bpp_wip_verify_batch (host pointers) at one proof and at a small block: first with no
    transcript, no challenges and no optional output, then with all of them -- the prover against pyref, the verifier
    against the verdicts pyref's proofs deserve and, in addition, against the device entry's scalars and sums"""
    import ctypes
    from bulletproofsplus_amd import _lib
    torch = need_gpu()
    cx = Ctx("secp256k1", 8, 1, 5)
    nv, k = 1, cx.k
    cases = [W.random_case(cx.pk, nv, 40 + i) for i in range(count)]
    a, b, y, g = [c.a for c in cases], [c.b for c in cases], [c.y for c in cases], [c.gamma for c in cases]
    stm = [c.statement() for c in cases]
    mine = np.stack([np.concatenate([cx.wire([c.A_prime]), np.zeros((2 + 2 * k, cx.PW), np.uint64), cx.wire(c.V)]) for c in cases])

    # absent: the literal challenges, verdicts alone
    rec, sc, ch = cx.bv.wip_prove_batch(a, b, y, g, nv, points=mine)
    for i, c in enumerate(cases):
        pf = c.prove()
        assert np.array_equal(rec[i, 1:3 + 2 * k], cx.wire([pf.A, pf.B] + list(pf.L_vec) + list(pf.R_vec))), i
        assert O.wire_to_scalars(sc[i]) == [pf.r_prime, pf.s_prime, pf.d_prime], i
        assert O.wire_to_scalars(ch[i]) == [99] + [7] * k
    assert np.array_equal(rec[:, 0], mine[:, 0]) and np.array_equal(rec[:, 3 + 2 * k:], mine[:, 3 + 2 * k:])
    # ... and without the challenges coming back (the wrapper always asks for them)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)
    av, bw = _rows_wire(a), _rows_wire(b)
    yv, gv = O.scalars_to_wire(y), O.scalars_to_wire(g)
    rec_raw, sc_raw = mine.copy(), np.zeros_like(sc)
    assert _lib.lib().bpp_wip_prove_batch(cx.bv.handle, vp(av), vp(bw), vp(yv), vp(gv), count, nv, 0, None, None, 0, None,
                                          vp(rec_raw), vp(sc_raw), None) == 0
    assert np.array_equal(rec_raw, rec) and np.array_equal(sc_raw, sc)
    assert cx.bv.wip_verify_batch(rec, sc, y, stm, nv).tolist() == [0] * count
    bad = sc.copy()
    bad[count - 1, 1, 0] ^= 1
    assert cx.bv.wip_verify_batch(rec, bad, y, stm, nv).tolist() == [0] * (count - 1) + [1]

    # present: the caller's transcript, the challenges out; the MulVec scalars and the sums out of the verifier
    states = [hashlib.sha256(b"host form %d" % i).digest() for i in range(count)]
    tr = np.frombuffer(b"".join(states), dtype=np.uint8).reshape(count, 32)
    rec, sc, ch = cx.bv.wip_prove_batch(a, b, y, g, nv, points=mine, transcript=tr)
    for i, c in enumerate(cases):
        pf, es = _pyref_fs_prove(cx, c, states[i])
        assert np.array_equal(rec[i, 1:3 + 2 * k], cx.wire([pf.A, pf.B] + list(pf.L_vec) + list(pf.R_vec))), i
        assert O.wire_to_scalars(sc[i]) == [pf.r_prime, pf.s_prime, pf.d_prime], i
        assert O.wire_to_scalars(ch[i]) == es, i
    ok, osc, ores = cx.bv.wip_verify_batch(rec, sc, y, stm, nv, transcript=tr, want_scalars=True, want_result=True)
    dok, dsc, dres = _verify_device(torch, cx, rec, sc, y, stm, nv, transcript=states)
    assert ok.tolist() == dok.tolist() == [0] * count
    assert np.array_equal(osc, dsc.reshape(osc.shape)) and np.array_equal(ores, dres.reshape(ores.shape))
    assert all(O.wire_to_point(cx.cid, ores[i]) is None for i in range(count))       # an accepted proof sums to the identity
    assert cx.bv.wip_verify_batch(rec, sc, y, stm, nv, challenges=[O.wire_to_scalars(c) for c in ch]).tolist() == [0] * count
    assert cx.bv.wip_verify_batch(rec, sc, y, stm, nv).tolist() == [1] * count       # the literals are not these challenges


# ---- 4. blinding -------------------------------------------------------------------------------------------------------
def _with_blinding(bl, k, f):
    T = P.Transcript
    saved = (T.R, T.S, T.DELTA, T.ETA, T.D_L, T.D_R)
    T.R, T.S, T.DELTA, T.ETA, T.D_L, T.D_R = bl[1], bl[2], bl[3], bl[4], bl[5], bl[5 + k]
    try:
        return f()
    finally:
        T.R, T.S, T.DELTA, T.ETA, T.D_L, T.D_R = saved


def test_blinding_from_a_key_and_from_a_buffer():
    torch = need_gpu()
    key = bytes(range(7, 39))
    # one round: the key's d_L[0], d_R[0] are all there is
    cx = Ctx("secp256k1", 2, 1, 5)
    c = W.random_case(cx.pk, 0, 41)
    st = [hashlib.sha256(b"blind 2").digest()]
    rec, sc, _ = _prove_device(torch, cx, [c.a], [c.b], [c.y], [c.gamma], 0, transcript=st, blind_key=key, index_base=500)
    bl = O.blinding_from_key(key, 500, cx.k, cx.r)
    pf, _ = _with_blinding(bl, cx.k, lambda: _pyref_fs_prove(cx, c, st[0]))
    assert np.array_equal(rec[0, 1:], cx.wire([pf.A, pf.B] + list(pf.L_vec) + list(pf.R_vec)))
    assert O.wire_to_scalars(sc[0]) == [pf.r_prime, pf.s_prime, pf.d_prime]
    # three rounds, a buffer whose d_L[t], d_R[t] are the same in every round (what pyref's class attributes express)
    cx = Ctx("secp256k1", 8, 1, 5)
    k = cx.k
    c = W.random_case(cx.pk, 1, 42)
    st = [hashlib.sha256(b"blind 8").digest()]
    rng = random.Random(43)
    base = [rng.randrange(1, cx.r) for _ in range(7)]
    bl = base[:5] + [base[5]] * k + [base[6]] * k
    rec, sc, _ = _prove_device(torch, cx, [c.a], [c.b], [c.y], [c.gamma], 1, transcript=st, blinding=[bl])
    pf, _ = _with_blinding(bl, k, lambda: _pyref_fs_prove(cx, c, st[0]))
    assert np.array_equal(rec[0, 1:3 + 2 * k], cx.wire([pf.A, pf.B] + list(pf.L_vec) + list(pf.R_vec)))
    assert O.wire_to_scalars(sc[0]) == [pf.r_prime, pf.s_prime, pf.d_prime]
    # the key at two index bases: different proofs, both valid
    recs, scs = [], []
    for ib in (0, 1 << 40):
        rec, sc, _ = _prove_device(torch, cx, [c.a], [c.b], [c.y], [c.gamma], 1, transcript=st, blind_key=key, index_base=ib)
        rec[0, 0], rec[0, 3 + 2 * k:] = cx.wire([c.A_prime])[0], cx.wire(c.V)
        recs.append(rec[0])
        scs.append(sc[0])
    assert not np.array_equal(recs[0], recs[1]) and not np.array_equal(scs[0], scs[1])
    ok, _, _ = _verify_device(torch, cx, np.stack(recs), np.stack(scs), [c.y] * 2, [c.statement()] * 2, 1, transcript=st * 2)
    assert ok.tolist() == [0, 0]


# ---- 4b. more proofs than one chunk of the prover's workspace ------------------------------------------------------------
def _bulk_wire(xs):
    """O.scalars_to_wire for thousands of scalars < 2^256"""
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()


def test_seam_across_a_chunk_boundary():
    """one call over 2050 proofs == the calls [0:2048] and [2048:2050], in literal mode, under the transcript with a key and
    with a blinding buffer; the proofs next to the boundary against pyref; the key's expansion against the oracle's"""
    torch = need_gpu()
    cx = Ctx("secp256k1", 8, 1, 5)
    k, r, ln, nv = cx.k, cx.r, cx.length, 1
    # The prover works through a batch in chunks of min(2048, 12 GB / (virtual proofs x MulVec length x 32 B)) proofs.  Here a
    # proof has 2k + 3 = 9 virtual proofs of 2 len + 2k + 5 = 27 scalars, 7.8 kB: the memory bound is six orders of
    # magnitude away and a chunk is 2048 proofs.
    chunk, count, base = 2048, 2050, 1000
    rng = random.Random(20480)
    a = [[rng.randrange(r) for _ in range(ln)] for _ in range(count)]
    b = [[rng.randrange(r) for _ in range(ln)] for _ in range(count)]
    y = [rng.randrange(1, r) for _ in range(count)]
    gamma = [rng.randrange(r) for _ in range(count)]
    wa = _bulk_wire([x for row in a for x in row]).reshape(count, ln, 4)
    wb = _bulk_wire([x for row in b for x in row]).reshape(count, ln, 4)
    wy, wg = _bulk_wire(y), _bulk_wire(gamma)
    states = [hashlib.sha256(b"chunk boundary %d" % i).digest() for i in range(count)]
    key = bytes(range(50, 82))
    # d_L[t], d_R[t] the same in every round: what pyref's class attributes express
    const_bl = []
    for _ in range(count):
        s7 = [rng.randrange(1, r) for _ in range(7)]
        const_bl.append(s7[:5] + [s7[5]] * k + [s7[6]] * k)
    w_const = _bulk_wire([x for row in const_bl for x in row]).reshape(count, 5 + 2 * k, 4)
    w_key = _bulk_wire([x for i in range(count) for x in O.blinding_from_key(key, base + i, k, r)]).reshape(count, 5 + 2 * k, 4)

    def run(lo, hi, **kw):
        return _prove_device(torch, cx, wa[lo:hi], wb[lo:hi], wy[lo:hi], wg[lo:hi], nv, **kw)

    modes = {
        "literal": lambda lo, hi: run(lo, hi),
        "key": lambda lo, hi: run(lo, hi, transcript=states[lo:hi], blind_key=key, index_base=base + lo),
        "buffer": lambda lo, hi: run(lo, hi, transcript=states[lo:hi], blinding=w_const[lo:hi]),
    }
    sent = np.frombuffer(bytes([SENT]) * 8, dtype=np.uint64)[0]
    near = (0, chunk - 1, chunk, count - 1)
    cases = {i: W.WipCase(cx.pk, a[i], b[i], y[i], gamma[i], None, None, None, None, [], None) for i in near}
    for name, f in modes.items():
        rec, sc, ch = f(0, count)
        parts = [f(0, chunk), f(chunk, count)]          # the second call in key mode: index_base = 3048
        assert np.array_equal(rec[:, 1:3 + 2 * k], np.concatenate([p[0][:, 1:3 + 2 * k] for p in parts])), name
        assert np.array_equal(sc, np.concatenate([p[1] for p in parts])), name
        assert np.array_equal(ch, np.concatenate([p[2] for p in parts])), name
        assert (rec[:, 0] == sent).all() and (rec[:, 3 + 2 * k:] == sent).all(), name      # A' and V are the caller's
        if name == "key":       # the oracle's expansion of the key, handed over as a buffer
            kr, ks, kc = run(0, count, transcript=states, blinding=w_key)
            assert np.array_equal(rec, kr) and np.array_equal(sc, ks) and np.array_equal(ch, kc)
            continue
        for i in near:
            if name == "literal":
                pf, es = cases[i].prove(), [99] + [7] * k
            else:
                pf, es = _with_blinding(const_bl[i], k, lambda: _pyref_fs_prove(cx, cases[i], states[i]))
            assert np.array_equal(rec[i, 1:3 + 2 * k], cx.wire([pf.A, pf.B] + list(pf.L_vec) + list(pf.R_vec))), (name, i)
            assert O.wire_to_scalars(sc[i]) == [pf.r_prime, pf.s_prime, pf.d_prime], (name, i)
            assert O.wire_to_scalars(ch[i]) == es, (name, i)


# ---- 5. the verifier equals the range pass, m = 1 --------------------------------------------------------------------
@pytest.mark.parametrize("cname,n", [("secp256k1", 8), ("bls12_381", 16)])
def test_verifier_equals_the_range_pass(cname, n):
    torch = need_gpu()
    cx = Ctx(cname, n, 1, 5)
    k, r = cx.k, cx.r
    names = list(W.TAMPERS)
    count = 1 + len(names)
    vals = [[(37 * i + 5) % (1 << n)] for i in range(count)]
    gams = [[1000003 * i + 17] for i in range(count)]
    pts, sc, V = cx.bv.prove_batch(vals, gams)
    rec = np.concatenate([pts, V], axis=1)
    y, z = P.Transcript.yz(1)
    stm0 = W.range_exponents(r, n, 1, y, z)
    stm = [list(stm0[0]) + list(stm0[1]) + [stm0[2]] + list(stm0[3]) for _ in range(count)]
    g = cx.cp.gh[0]
    idx = {"A_prime": 0, "wip_A": 1, "L0": 3, "R_last": 3 + 2 * k - 1, "V0": 3 + 2 * k}
    stm_idx = {"Gc_last": n - 1, "Hc0": n, "gc": 2 * n, "Vc0": 2 * n + 1}
    for j, name in enumerate(names, start=1):
        if name in idx:
            rec[j, idx[name]] = O.point_add(cx.cid, rec[j, idx[name]], g)
        elif name in ("r_prime", "s_prime", "d_prime"):
            sc[j, ("r_prime", "s_prime", "d_prime").index(name), 0] ^= 1
        else:
            stm[j][stm_idx[name]] = (stm[j][stm_idx[name]] + 1) % r
    ok, osc, ores = _verify_device(torch, cx, rec, sc, [y] * count, stm, 1)
    rok, rsc, rres = run_verifier_device(torch, cx.bv, rec, sc)
    nstm = count - 4                     # the statement tampers are the last four: bpp_verifier_run cannot see them
    assert ok[:nstm].tolist() == rok[:nstm].tolist() == [0] + [1] * (nstm - 1)
    assert np.array_equal(osc[:nstm], rsc[:nstm])
    assert np.array_equal(ores[:nstm], rres[:nstm])
    assert ok[nstm:].tolist() == [1, 1, 1, 1] and rok[nstm:].tolist() == [0, 0, 0, 0]
    # each statement tamper moves exactly the scalar it feeds (MulVec order), by e^2
    N, e2 = 2 * n + 2 * k + 6, 99 * 99
    where = {"Gc_last": 5 + 2 * k + n - 1, "Hc0": 5 + 2 * k + n, "gc": 3, "Vc0": N - 1}
    for j in range(nstm, count):
        diff = [t for t in range(N) if not np.array_equal(osc[j, t], rsc[j, t])]
        assert diff == [where[names[j - 1]]], names[j - 1]
        t = diff[0]
        assert (O.limbs_to_int(osc[j, t]) - O.limbs_to_int(rsc[j, t])) % r == e2


# ---- 6. aggregated range proofs through the seam ---------------------------------------------------------------------
def test_aggregated_range_proofs_through_the_seam():
    torch = need_gpu()
    n, m = 4, 4
    cx = Ctx("bls12_381", n, m, 5)
    k, count = cx.k, 9
    vals = [[(3 * i + j) % 16 for j in range(m)] for i in range(count)]
    gams = [[100 * i + j + 1 for j in range(m)] for i in range(count)]
    pts, sc, V = cx.bv.prove_batch(vals, gams)
    rec = np.concatenate([pts, V], axis=1)
    g = cx.cp.gh[0]
    rec[2, 3] = O.point_add(cx.cid, rec[2, 3], g)               # L_0
    sc[5, 2, 0] ^= 1                                            # delta'
    rec[7, 3 + 2 * k + 3] = O.point_add(cx.cid, rec[7, 3 + 2 * k + 3], g)   # V_3
    y, z = P.Transcript.yz(m)
    e = W.range_exponents(cx.r, n, m, y, z)
    stm = [list(e[0]) + list(e[1]) + [e[2]] + list(e[3])] * count
    ok, _, _ = _verify_device(torch, cx, rec, sc, [y] * count, stm, m)
    rok, _, _ = run_verifier_device(torch, cx.bv, rec, sc, want_scalars=False, want_result=False)
    assert ok.tolist() == rok.tolist() == [0, 0, 1, 0, 0, 1, 0, 1, 0]


# ---- 7. geometry sweep ---------------------------------------------------------------------------------------------------
def _sweep_cases(cx, nv, count, seed):
    """statements whose A' is a short MulVec (so that hundreds of them cost the oracle little) and still bind every
    Gc[i], Hc[i]: Gc = a, Hc = b except at two indices each, V_j = t_j g.  -> a, b, y, gamma, statements, A' wire, V wire"""
    rng = random.Random(seed)
    r, n = cx.r, cx.length
    g, h = cx.pk.g, cx.pk.h
    ts = [rng.randrange(1, r) for _ in range(nv)]
    V = [cx.msm([t], [g]) for t in ts]
    out = dict(a=[], b=[], y=[], gamma=[], stm=[], Ap=[])
    for _ in range(count):
        a = [rng.randrange(r) for _ in range(n)]
        b = [rng.randrange(r) for _ in range(n)]
        y, gamma = rng.randrange(1, r), rng.randrange(r)
        Gc, Hc = list(a), list(b)
        ig, ih = sorted({0, rng.randrange(n)}), sorted({n - 1, rng.randrange(n)})
        du = {i: rng.randrange(1, r) for i in ig}
        dv = {i: rng.randrange(1, r) for i in ih}
        for i, d in du.items():
            Gc[i] = (a[i] - d) % r
        for i, d in dv.items():
            Hc[i] = (b[i] - d) % r
        gc = rng.randrange(r)
        Vc = [rng.randrange(1, r) for _ in range(nv)]
        c, yp = 0, 1
        for i in range(n):
            yp = yp * y % r
            c = (c + a[i] * b[i] % r * yp) % r
        gs = (c - gc - sum(vc * t for vc, t in zip(Vc, ts))) % r
        Ap = cx.msm(list(du.values()) + list(dv.values()) + [gs, gamma],
                    [cx.pk.G_vec[i] for i in du] + [cx.pk.H_vec[i] for i in dv] + [g, h])
        for key, val in (("a", a), ("b", b), ("y", y), ("gamma", gamma), ("stm", Gc + Hc + [gc] + Vc), ("Ap", Ap)):
            out[key].append(val)
    return out, V


@pytest.mark.parametrize("cname,n,m,nv,wb,count", [("bls12_381", 4, 1, 0, 3, 1), ("bls12_381", 64, 2, 3, 4, 70),
                                                   ("secp256k1", 64, 1, 1, 9, 300), ("ed25519", 16, 1, 2, 6, 40)])
def test_geometry_sweep(cname, n, m, nv, wb, count):
    torch = need_gpu()
    cx = Ctx(cname, n, m, wb)
    k, r, ln = cx.k, cx.r, cx.length
    cs, V = _sweep_cases(cx, nv, count, 7000 + ln)
    rec, sc, _ = _prove_device(torch, cx, cs["a"], cs["b"], cs["y"], cs["gamma"], nv)
    rec[:, 0] = cx.wire(cs["Ap"])
    if nv:
        rec[:, 3 + 2 * k:] = cx.wire(V)
    g = cx.cp.gh[0]
    expect = [0] * count
    fields = ("A_prime", "L0", "r_prime", "Gc_last", "wip_A", "d_prime", "Hc0", "R_last", "s_prime", "gc")
    stm = [list(s) for s in cs["stm"]]
    for t, j in enumerate(range(6, count, 7)):        # every seventh proof, a rotating field
        f = fields[t % len(fields)]
        expect[j] = 1
        pi = {"A_prime": 0, "wip_A": 1, "L0": 3, "R_last": 3 + 2 * k - 1}
        if f in pi:
            rec[j, pi[f]] = O.point_add(cx.cid, rec[j, pi[f]], g) if cname != "ed25519" else cx.wire(
                [cx.cp.grp.add(O.wire_to_point(2, rec[j, pi[f]]), cx.pk.g)])[0]
        elif f in ("r_prime", "s_prime", "d_prime"):
            sc[j, ("r_prime", "s_prime", "d_prime").index(f), 0] ^= 1
        else:
            si = {"Gc_last": ln - 1, "Hc0": ln, "gc": 2 * ln}[f]
            stm[j][si] = (stm[j][si] + 1) % r
    ok, osc, ores = _verify_device(torch, cx, rec, sc, cs["y"], stm, nv)
    assert ok.tolist() == expect
    # scalars against pyref's verify_mulvec (a scalar list: the shadow group carries it), result against the oracle's MulVec
    spk = P.PublicKey(P.ShadowGroup(r), ln)
    fixed = [cx.pk.g, cx.pk.h]
    for j in sorted({0, count // 2, count - 1} | ({6} if count > 6 else set())):
        s3 = O.wire_to_scalars(sc[j])
        pf = P.WeightedInnerProductProof([0] * k, [0] * k, 0, 0, s3[0] % r, s3[1] % r, s3[2] % r)
        F = P.Fr(r)
        mv = pf.verify_mulvec(spk, F.exp_iter_type2(cs["y"][j], ln), stm[j][:ln], stm[j][ln:2 * ln], stm[j][2 * ln],
                              stm[j][2 * ln + 1:], 0, [0] * nv)
        assert O.wire_to_scalars(osc[j]) == mv.scalars, j
        pts = O.wire_to_points(cx.cid, rec[j])
        order = [pts[2], pts[1], pts[0]] + fixed + pts[3:3 + 2 * k] + list(cx.pk.G_vec) + list(cx.pk.H_vec) + pts[3 + 2 * k:]
        res = cx.msm(mv.scalars, order)
        assert O.wire_to_point(cx.cid, ores[j]) == res, j
        assert (res is None) == (expect[j] == 0), j


# ---- 8. subgroup check, usage errors and y = 0 on a live engine -------------------------------------------------------
def test_subgroup_check_errors_and_zero_y():
    torch = need_gpu()
    B = __import__("bulletproofsplus_amd")
    cx = Ctx("bls12_381", 8, 1, 5)
    k, nv = cx.k, 1
    cs, V = _sweep_cases(cx, nv, 4, 88)
    cs["y"][2] = cx.r                                   # = 0 (mod r)
    rec, sc, _ = _prove_device(torch, cx, cs["a"], cs["b"], cs["y"], cs["gamma"], nv)
    rec[:, 0] = cx.wire(cs["Ap"])
    rec[:, 3 + 2 * k:] = cx.wire(V)
    ok, _, _ = _verify_device(torch, cx, rec, sc, cs["y"], cs["stm"], nv)
    assert ok.tolist() == [0, 0, 1, 0]
    # L_0 + T, T = (0, 2) of order 3: the MulVec scalar of L_0 decides without the check, the check rejects it
    shifted = rec.copy()
    shifted[0, 3] = cx.wire([cx.cp.grp.add(O.wire_to_point(0, rec[0, 3]), VC.bls_T())])[0]
    cx.bv.set_subgroup_check(True)
    try:
        ok, _, _ = _verify_device(torch, cx, shifted, sc, cs["y"], cs["stm"], nv)
    finally:
        cx.bv.set_subgroup_check(False)
    assert ok.tolist() == [1, 0, 1, 0]
    # usage errors: BPP_E_ARG, d_ok untouched
    full = cx.bv.wip_verifier_workspace_bytes(4, nv)
    for kw in (dict(wsb=full - 1), dict(flags_transcript=True)):
        with pytest.raises(B.BppError) as ei:
            _verify_device(torch, cx, rec, sc, cs["y"], cs["stm"], nv, **kw)
        assert ei.value.code == -1
    assert cx.bv.wip_verifier_workspace_bytes(4, 65) == 0
    d = torch.full((64,), 7, dtype=torch.int32, device="cuda:0")
    p = d.data_ptr()
    with pytest.raises(B.BppError) as ei:
        cx.bv.wip_verify_device(p, p, p, p, 65, 4, p, p, 1 << 30)
    assert ei.value.code == -1
    with pytest.raises(B.BppError):
        cx.bv.wip_prove_device(p, p, p, p, 4, nv, p, p, p, cx.bv.wip_prover_workspace_bytes(4) - 1)
    with pytest.raises(B.BppError):
        cx.bv.wip_prove_device(p, p, p, p, 4, nv, p, p, p, 1 << 30, blind_key=bytes(32))
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == 7).all()


# ---- 9. the Python mirror -------------------------------------------------------------------------------------------------
def test_python_mirror_round_trip():
    need_gpu()
    cx = Ctx("secp256k1", 8, 1, 4)
    B = cx.B
    bpk = B.PublicKey.from_points(cx.a, cx.cp.gh, cx.cp.G, cx.cp.H)
    c = W.random_case(cx.pk, 2, 91)
    pw = c.powers()
    pf = B.WeightedInnerProductProof.prove(bpk, c.a, c.b, pw, c.gamma, None)
    ref = c.prove()
    assert np.array_equal(np.stack([pf.A, pf.B]), cx.wire([ref.A, ref.B]))
    Ap, V = cx.wire([c.A_prime])[0], cx.wire(c.V)
    assert pf.verify(bpk, pw, c.Gc, c.Hc, c.gc, c.Vc, Ap, V) is None
    assert pf.verify(bpk, pw, c.Gc, c.Hc, c.gc, c.Vc, Ap, V, engine=cx.bv) is None
    with pytest.raises(B.VerificationError):
        pf.verify(bpk, pw, c.Gc, c.Hc, (c.gc + 1) % cx.r, c.Vc, Ap, V, engine=cx.bv)
    with pytest.raises(ValueError):
        pf.verify(bpk, pw[:-1] + [pw[-1] + 1], c.Gc, c.Hc, c.gc, c.Vc, Ap, V, engine=cx.bv)
    with pytest.raises(ValueError):
        B.WeightedInnerProductProof.prove(bpk, c.a, c.b, [1] + pw[:-1], c.gamma, None, engine=cx.bv)


def test_cpp_mirror_round_trip(tmp_path):
    """include/bpp_amd.hpp: the two members of bpp::WeightedInnerProductProof prove, verify and reject a tamper"""
    need_gpu()
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "wip_mirror_main")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(root, "tests", "host", "wip_mirror_main.cpp"),
                           "-L" + os.path.join(root, "bulletproofsplus_amd"), "-lbpp_amd",
                           "-Wl,-rpath," + os.path.join(root, "bulletproofsplus_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "verify=Ok(())" in out.stdout and "tampered=Err(VerificationError)" in out.stdout
