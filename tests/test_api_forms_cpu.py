"""CPU: what the Python front of the host forms (bulletproofsplus_amd/api.py) checks, what it hands to the C ABI and what
it makes of the answer -- no GPU, no engine handle.

`_lib.lib` is replaced by a recorder: the pure getters (sizes, bpp_proofs_scan, bpp_shard_cuts, bpp_last_error) go to
the real library, every other entry is recorded as (name, args) and answers with a code and output words the test
chooses.  `api._ptr`, the one doorway from arrays to pointers, is replaced by the identity, so the recorder sees the
arrays themselves (copied at call time) or None.  The verifier and the pool are built with __new__ around integer handles
that never reach native code.

Shapes: n = 8, capacity m = 4, ms = [1, 2, 4, 1] (three aggregation classes, one repeated), two keys; secp256k1 and
BLS12-381 because their point sizes differ.  Every byte count comes from the library's getters."""

import contextlib
import ctypes
import itertools
import types

import numpy as np
import pytest

from bulletproofsplus_amd import _lib, api

N, M, MS = 8, 4, [1, 2, 4, 1]
COUNT, N_OUT = len(MS), sum(MS)
KEYS = [bytes(range(32)), bytes(range(100, 132))]
H, AH, PH = 0xB1, 0xA1, 0xC1   # verifier, context and pool "handles"
A64, SEALED = 0x100, 0x200     # BPP_PROVE_AMOUNT64, BPP_FIND_AMOUNTS_SEALED (include/bpp_amd.h)
PURE = ("bpp_proof_bytes_version", "bpp_proof_bytes", "bpp_point_compressed_bytes", "bpp_point_uncompressed_bytes",
        "bpp_proofs_scan", "bpp_shard_cuts", "bpp_last_error")
BOOLS = (False, True)


def u8(x):
    return np.asarray(x, dtype=np.uint8)


def u32(x):
    return np.asarray(x, dtype=np.uint32)


def u64(x):
    return np.asarray(x, dtype=np.uint64)


def limbs(x):
    return [(x >> (64 * i)) & (2 ** 64 - 1) for i in range(4)]


def log2(x):
    return x.bit_length() - 1


def points_of(m):
    return 3 + 2 * log2(N * m) + m


class Is:
    """an expected argument given as a predicate"""

    def __init__(self, pred):
        self.pred = pred


KEY32 = Is(lambda g: type(g) is bytes and len(g) == 32)
STATS = Is(lambda g: isinstance(g, ctypes.Array) and len(g) == 2)


class Recorder:
    def __init__(self, real, real_ptr):
        self.real, self.real_ptr = real, real_ptr
        self.calls = []    # (name, args as copied at call time)
        self.live = {}     # name -> the argument objects themselves
        self.rc = {}       # name -> return code (default 0)
        self.writes = {}   # name -> {argument position: words written before returning}

    def __getattr__(self, name):
        if name in PURE:
            f = getattr(self.real, name)
            return lambda *a: f(*[self.real_ptr(x) if isinstance(x, np.ndarray) else x for x in a])

        def entry(*args):
            self.calls.append((name, [a.copy() if isinstance(a, np.ndarray) else
                                      int(a.value) if isinstance(a, ctypes.c_uint64) else a for a in args]))
            self.live[name] = args
            for pos, words in self.writes.get(name, {}).items():
                if args[pos] is None:
                    continue
                out =args[pos].reshape(-1) if isinstance(args[pos], np.ndarray) else args[pos]
                for i in range(min(len(out), len(words))):
                    out[i] = words[i]
            return self.rc.get(name, 0)
        return entry


class Rig:
    def __init__(self, curve, rec):
        self.curve, self.rec = curve, rec
        L = _lib.FP_LIMBS[curve]
        self.PW = 2 * L + 1
        self.arith = types.SimpleNamespace(curve=curve, L=L, PW=self.PW, handle=AH)
        self.bv = api.BatchVerifier.__new__(api.BatchVerifier)
        self.bv.arith, self.bv.n, self.bv.m, self.bv.handle, self.bv._owner = self.arith, N, M, H, self
        self.pool = api.VerifierPool.__new__(api.VerifierPool)
        self.pool.arith, self.pool.n, self.pool.m, self.pool.handle = self.arith, N, M, PH

    def point_bytes(self, unc):
        return (self.rec.real.bpp_point_uncompressed_bytes if unc else self.rec.real.bpp_point_compressed_bytes)(self.curve)

    def proof_bytes(self, m, unc):
        return self.rec.real.bpp_proof_bytes_version(self.curve, N, m, 2 if unc else 1)

    def stream(self, ms, unc):
        """zero-filled containers of the right lengths behind the 9 header bytes the framing reads"""
        return b"".join(b"BPP+" + bytes([2 if unc else 1, self.curve, N, m, log2(N * m)]) + bytes(self.proof_bytes(m, unc) - 9)
                        for m in ms)

    def commitments(self, ms, unc):
        return bytes(range(7, 7 + sum(ms))) * self.point_bytes(unc)

    def one(self, name, want):
        """exactly one recorded call, of this name, with these arguments (dtype, shape and contents for arrays)"""
        assert [c[0] for c in self.rec.calls] == [name]
        got = self.rec.calls[0][1]
        self.rec.calls.clear()
        assert len(got) == len(want), (len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            if isinstance(w, Is):
                assert w.pred(g), (name, i, g)
            elif isinstance(w, np.ndarray):
                assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), \
                    (name, i, g, w)
            else:
                assert type(g) is type(w) and g == w, (name, i, g, w)

    @contextlib.contextmanager
    def refuses(self, exc, text):
        """a usage error: this type, this whole text, before anything is handed to the library"""
        self.rec.calls.clear()
        with pytest.raises(exc) as e:
            yield
        assert type(e.value) is exc and str(e.value) == text
        assert self.rec.calls == []


@pytest.fixture(params=[_lib.SECP256K1, _lib.BLS12_381_G1], ids=["secp256k1", "bls12_381"])
def rig(request, monkeypatch):
    real = _lib.lib()
    rec = Recorder(real, api._ptr)
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(api, "_ptr", lambda a: a)
    r = Rig(request.param, rec)
    yield r
    r.bv.handle = r.pool.handle = None   # nothing for close() to hand to the real library


def flag_cases(*names):
    """every combination of the named booleans -> (kwargs, flag word)"""
    bit = {"transcript": 1, "uncompressed": 2, "amount64": A64, "sealed": SEALED}
    for combo in itertools.product(BOOLS, repeat=len(names)):
        yield dict(zip(names, combo)), sum(bit[n] for n, on in zip(names, combo) if on)


def packed_keys():
    return u8(list(b"".join(KEYS)))


HIT_WORDS = [1, 3, 0x89ABCDEF, 0x01234567, 11, 12, 13, 14, 15, 16, 17, 0x80000000,
             0, 2, 5, 0, 1, 0, 0, 0, 0, 0, 0, 0]
HITS = [(1, 3, 0x0123456789ABCDEF, 11 | 12 << 32 | 13 << 64 | 14 << 96 | 15 << 128 | 16 << 160 | 17 << 192 | 0x80000000 << 224),
        (0, 2, 5, 1)]


# ---- the verify forms ----
def test_verify_wire_mixed(rig):
    bv, PW = rig.bv, rig.PW
    recs = [np.arange(points_of(m) * PW, dtype=np.uint64).reshape(-1, PW) + 1000 * i for i, m in enumerate(MS)]
    packed = np.concatenate(recs)
    sc = np.arange(COUNT * 12, dtype=np.uint64).reshape(COUNT, 3, 4)
    rig.rec.writes["bpp_range_verify_batch_mixed"] = {5: [0, 1, 2, 0]}
    for records in (recs, tuple(recs), packed, packed.reshape(-1)):
        ok = bv.verify_wire_mixed(records, sc, MS)
        rig.one("bpp_range_verify_batch_mixed", [H, packed, sc, u32(MS), COUNT, np.zeros(COUNT, np.uint32)])
        assert ok.dtype == np.uint32 and ok.tolist() == [0, 1, 2, 0]
    # count = 0: arrays all the same, none of them None
    for records in ([], np.zeros((0, PW), np.uint64)):
        assert bv.verify_wire_mixed(records, np.zeros((0, 3, 4), np.uint64), []).shape == (0,)
        rig.one("bpp_range_verify_batch_mixed", [H, np.zeros((0, PW), np.uint64), np.zeros((0, 3, 4), np.uint64), u32([]), 0,
                                                 np.zeros(0, np.uint32)])
    # an m_i the verifier does not take: nothing is checked here, the library names the proof
    for bad in (3, 8, 0):
        bv.verify_wire_mixed(packed[:5], sc[:2], [1, bad])
        rig.one("bpp_range_verify_batch_mixed", [H, packed[:5], sc[:2], u32([1, bad]), 2, np.zeros(2, np.uint32)])
        bv.verify_wire_mixed([packed[:1], packed[:2]], sc[:2], [1, bad])
        rig.one("bpp_range_verify_batch_mixed", [H, packed[[0, 0, 1]], sc[:2], u32([1, bad]), 2, np.zeros(2, np.uint32)])
    with rig.refuses(RuntimeError, "verify_wire_mixed: one record per entry of ms"):
        bv.verify_wire_mixed(recs[:3], sc, MS)
    with rig.refuses(RuntimeError, "verify_wire_mixed: record 2 does not hold %d points" % points_of(4)):
        bv.verify_wire_mixed(recs[:2] + [recs[2][:-1]] + recs[3:], sc, MS)
    with rig.refuses(RuntimeError, "verify_wire_mixed: %d wire points, the shapes in ms need %d" % (len(packed) - 1, len(packed))):
        bv.verify_wire_mixed(packed[:-1], sc, MS)
    with rig.refuses(RuntimeError, "verify_wire_mixed: one scalar triple per proof record"):
        bv.verify_wire_mixed(packed, sc[:3], MS)


def test_pool_verify_wire_mixed(rig):
    pool, PW = rig.pool, rig.PW
    recs = [np.arange(points_of(m) * PW, dtype=np.uint64).reshape(-1, PW) + 1000 * i for i, m in enumerate(MS)]
    packed = np.concatenate(recs)
    sc = np.arange(COUNT * 12, dtype=np.uint64).reshape(COUNT, 3, 4)
    rig.rec.writes["bpp_pool_verify_mixed"] = {5: [0, 1, 2, 0]}
    for records in (recs, packed):
        ok = pool.verify_wire_mixed(records, sc, MS)
        rig.one("bpp_pool_verify_mixed", [PH, packed, sc, u32(MS), COUNT, np.zeros(COUNT, np.uint32)])
        assert ok.dtype == np.uint32 and ok.tolist() == [0, 1, 2, 0]
    # ms None: a uniform batch at the capacity shape
    uni = np.arange(2 * points_of(M) * PW, dtype=np.uint64).reshape(2, points_of(M), PW)
    pool.verify_wire_mixed(uni, sc[:2])
    rig.one("bpp_pool_verify_mixed", [PH, uni.reshape(-1, PW), sc[:2], None, 2, np.zeros(2, np.uint32)])
    pool.verify_wire_mixed([], np.zeros((0, 3, 4), np.uint64), [])
    rig.one("bpp_pool_verify_mixed", [PH, np.zeros((0, PW), np.uint64), np.zeros((0, 3, 4), np.uint64), u32([]), 0,
                                      np.zeros(0, np.uint32)])
    for bad in (3, 8, 0):
        pool.verify_wire_mixed(packed[:5], sc[:2], [1, bad])
        rig.one("bpp_pool_verify_mixed", [PH, packed[:5], sc[:2], u32([1, bad]), 2, np.zeros(2, np.uint32)])
    with rig.refuses(RuntimeError, "verify_wire_mixed: one scalar triple per entry of ms"):
        pool.verify_wire_mixed(packed, sc[:3], MS)
    with rig.refuses(RuntimeError, "verify_wire_mixed: %d wire points, the shapes need %d" % (len(packed) - 1, len(packed))):
        pool.verify_wire_mixed(packed[:-1], sc, MS)
    with rig.refuses(RuntimeError, "verify_wire_mixed: %d wire points, the shapes need %d" % (1, 2 * points_of(M))):
        pool.verify_wire_mixed(packed[:1], sc[:2])


def test_verify_serialized_mixed(rig):
    bv, name = rig.bv, "bpp_range_verify_batch_serialized_mixed"
    rig.rec.writes[name] = {6: [0, 1, 2, 0]}
    for kw, flags in flag_cases("transcript", "uncompressed"):
        unc = kw["uncompressed"]
        raw, cm = rig.stream(MS, unc), rig.commitments(MS, unc)
        assert len(cm) == N_OUT * rig.point_bytes(unc)
        want = [H, u8(list(raw)), u8(list(cm)), u32(MS), COUNT, flags, np.zeros(COUNT, np.uint32)]
        for proofs, ms in ((raw, MS), (raw, None), (bytearray(raw), u32(MS)), (u8(list(raw)), None)):
            ok = bv.verify_serialized_mixed(proofs, cm, ms, **kw)
            rig.one(name, want)
            assert ok.dtype == np.uint32 and ok.tolist() == [0, 1, 2, 0]
        with rig.refuses(RuntimeError, "verify_serialized_mixed: %d bytes of proofs, the shapes in ms need %d"
                         % (len(raw) - 1, len(raw))):
            bv.verify_serialized_mixed(raw[:-1], cm, MS, **kw)
        with rig.refuses(RuntimeError, "verify_serialized_mixed: ms[i] commitments per proof"):
            bv.verify_serialized_mixed(raw, cm[:-1], None, **kw)
    # count = 0, with ms given and with the empty stream framed
    for ms in ([], None):
        assert bv.verify_serialized_mixed(b"", b"", ms).shape == (0,)
        rig.one(name, [H, None, None, None, 0, 0, None])
    raw, cm = rig.stream(MS, False), rig.commitments(MS, False)
    for bad in (3, 8, 0):
        bv.verify_serialized_mixed(raw[:-1], cm[:-1], [1, bad])
        rig.one(name, [H, u8(list(raw[:-1])), u8(list(cm[:-1])), u32([1, bad]), 2, 0, np.zeros(2, np.uint32)])
    # a stream that cannot be framed is the library's error
    with pytest.raises(api.BppError):
        bv.verify_serialized_mixed(raw[:-1], cm)
    assert rig.rec.calls == []


def test_pool_verify_serialized_mixed(rig):
    pool, name = rig.pool, "bpp_pool_verify_serialized_mixed"
    rig.rec.writes[name] = {10: [0, 1, 2, 0], 11: [5, 9]}
    wk = bytes(range(50, 82))
    for kw, flags in flag_cases("transcript", "uncompressed"):
        unc = kw["uncompressed"]
        raw, cm = rig.stream(MS, unc), rig.commitments(MS, unc)
        head = [PH, u8(list(raw)), u8(list(cm)), u32(MS), COUNT, flags]
        for ms in (MS, None):
            ok = pool.verify_serialized_mixed(raw, cm, ms, **kw)
            rig.one(name, head + [0, None, 0, 0, np.zeros(COUNT, np.uint32), STATS])
            assert ok.dtype == np.uint32 and ok.tolist() == [0, 1, 2, 0]
        # ungrouped: key, group and stats are dropped whatever the caller gave
        pool.verify_serialized_mixed(raw, cm, MS, weight_key=wk, index_base=7, group=8, **kw)
        rig.one(name, head + [0, None, 7, 0, np.zeros(COUNT, np.uint32), STATS])
        ok, stats = pool.verify_serialized_mixed(raw, cm, MS, grouped=True, weight_key=wk, index_base=1 << 40, group=8,
                                                 return_stats=True, **kw)
        rig.one(name, head + [1, wk, 1 << 40, 8, np.zeros(COUNT, np.uint32), STATS])
        assert ok.tolist() == [0, 1, 2, 0] and stats == (5, 9)
        pool.verify_serialized_mixed(raw, cm, MS, grouped=True, **kw)
        rig.one(name, head + [1, KEY32, 0, 32, np.zeros(COUNT, np.uint32), STATS])
        with rig.refuses(RuntimeError, "verify_serialized_mixed: %d bytes of proofs, the shapes in ms need %d"
                         % (len(raw) - 1, len(raw))):
            pool.verify_serialized_mixed(raw[:-1], cm, MS, **kw)
        with rig.refuses(RuntimeError, "verify_serialized_mixed: ms[i] commitments per proof"):
            pool.verify_serialized_mixed(raw, cm[:-1], **kw)
    for ms in ([], None):
        assert pool.verify_serialized_mixed(b"", b"", ms).shape == (0,)
        rig.one(name, [PH, None, None, None, 0, 0, 0, None, 0, 0, None, STATS])
    raw, cm = rig.stream(MS, False), rig.commitments(MS, False)
    for bad in (3, 8, 0):
        pool.verify_serialized_mixed(raw[:-1], cm[:-1], [1, bad])
        rig.one(name, [PH, u8(list(raw[:-1])), u8(list(cm[:-1])), u32([1, bad]), 2, 0, 0, None, 0, 0, np.zeros(2, np.uint32), STATS])
    with rig.refuses(ValueError, "weight_key must be 32 bytes"):
        pool.verify_serialized_mixed(raw, cm, MS, grouped=True, weight_key=bytes(31))


# ---- mask recovery and the single-key scan ----
K_OF = [log2(N * m) for m in MS]
BLINDING = [[1000 * i + j for j in range(5 + 2 * k)] for i, k in enumerate(K_OF)]
BLINDING_WIRE = u64([limbs(x) for row in BLINDING for x in row])


def test_recover_masks(rig):
    bv, name = rig.bv, "bpp_range_recover_masks_mixed"
    sc = np.arange(COUNT * 12, dtype=np.uint64).reshape(COUNT, 3, 4)
    chs = [np.arange((3 + k) * 4, dtype=np.uint64).reshape(-1, 4) + 100 * i for i, k in enumerate(K_OF)]
    ch = np.concatenate(chs)
    key = bytes(range(32))
    masks = [5, 1 << 255 | 9, 0, (1 << 64) + 1]
    rig.rec.writes[name] = {9: [w for x in masks for w in limbs(x)]}
    out0 = np.zeros((COUNT, 4), np.uint64)
    assert bv.recover_masks(sc, MS) == masks
    rig.one(name, [H, sc, u32(MS), COUNT, None, None, 0, None, None, out0])
    for challenges in (chs, tuple(chs), ch, ch.reshape(-1)):
        assert bv.recover_masks(sc.reshape(-1), MS, challenges, blind_key=key, index_base=1 << 63) == masks
        rig.one(name, [H, sc, u32(MS), COUNT, ch, key, 1 << 63, None, None, out0])
    bv.recover_masks(sc, MS, blind_key=key, index=[9, 8, 7, 1 << 63], index_base=3)
    rig.one(name, [H, sc, u32(MS), COUNT, None, key, 3, u64([9, 8, 7, 1 << 63]), None, out0])
    for blinding in (BLINDING, BLINDING_WIRE, BLINDING_WIRE.reshape(-1)):
        bv.recover_masks(sc, MS, chs, blinding=blinding)
        rig.one(name, [H, sc, u32(MS), COUNT, ch, None, 0, None, BLINDING_WIRE, out0])
    assert bv.recover_masks(np.zeros((0, 3, 4), np.uint64), []) == []
    rig.one(name, [H, None, None, 0, None, None, 0, None, None, None])
    for bad in (3, 8, 0):   # no total to hold the challenges or the blinding against
        bv.recover_masks(sc[:2], [1, bad], ch[:3], blinding=BLINDING_WIRE[:2])
        rig.one(name, [H, sc[:2], u32([1, bad]), 2, ch[:3], None, 0, None, BLINDING_WIRE[:2], np.zeros((2, 4), np.uint64)])
    with rig.refuses(RuntimeError, "recover_masks: one scalar triple per proof"):
        bv.recover_masks(sc[:3], MS)
    with rig.refuses(RuntimeError, "recover_masks: 3 + k_i challenges per proof (%d in all), got %d" % (len(ch), len(ch) - 1)):
        bv.recover_masks(sc, MS, ch[:-1])
    with rig.refuses(RuntimeError, "one index per proof"):
        bv.recover_masks(sc, MS, blind_key=key, index=[1, 2, 3])
    with rig.refuses(RuntimeError, "blinding: 5 + 2 k_i scalars per proof (%d in all), got %d"
                     % (len(BLINDING_WIRE), len(BLINDING_WIRE) - 1)):
        bv.recover_masks(sc, MS, blinding=BLINDING_WIRE[:-1])
    with rig.refuses(ValueError, "blind_key: 32 bytes"):
        bv.recover_masks(sc, MS, blind_key=bytes(31))


def test_scan_serialized_mixed(rig):
    bv, name = rig.bv, "bpp_range_scan_serialized_mixed"
    key = bytes(range(32))
    masks = [5, 1 << 255 | 9, 0, (1 << 64) + 1]
    rig.rec.writes[name] = {11: [w for x in masks for w in limbs(x)], 12: [0, 3, 2, 1]}
    m0, s0 = np.zeros((COUNT, 4), np.uint64), np.zeros(COUNT, np.uint32)
    for kw, flags in flag_cases("transcript", "uncompressed", "amount64"):
        unc = kw["uncompressed"]
        raw, cm = rig.stream(MS, unc), rig.commitments(MS, unc)
        head = [H, u8(list(raw)), u8(list(cm)), u32(MS), COUNT, flags]
        for ms in (MS, None):
            status, got = bv.scan_serialized_mixed(raw, cm, ms, **kw)
            rig.one(name, head + [None, 0, None, None, None, m0, s0])
            assert status.dtype == np.uint32 and status.tolist() == [0, 3, 2, 1] and got == masks
        bv.scan_serialized_mixed(raw, cm, MS, blind_key=key, index_base=1 << 63, index=range(4), blinding=BLINDING,
                                 amounts=[1, 2, 3, 1 << 63], **kw)
        rig.one(name, head + [key, 1 << 63, u64([0, 1, 2, 3]), BLINDING_WIRE, u64([1, 2, 3, 1 << 63]), m0, s0])
        with rig.refuses(RuntimeError, "scan_serialized_mixed: %d bytes of proofs, the shapes in ms need %d"
                         % (len(raw) - 1, len(raw))):
            bv.scan_serialized_mixed(raw[:-1], cm, MS, **kw)
        with rig.refuses(RuntimeError, "scan_serialized_mixed: ms[i] commitments per proof"):
            bv.scan_serialized_mixed(raw, cm[:-1], **kw)
    for ms in ([], None):
        status, got = bv.scan_serialized_mixed(b"", b"", ms, index=[], amounts=[])
        rig.one(name, [H, None, None, None, 0, 0, None, 0, u64([]), None, u64([]), None, None])
        assert status.shape == (0,) and got == []
    raw, cm = rig.stream(MS, False), rig.commitments(MS, False)
    for bad in (3, 8, 0):
        bv.scan_serialized_mixed(raw[:-1], cm[:-1], [1, bad], blinding=BLINDING_WIRE[:1])
        rig.one(name, [H, u8(list(raw[:-1])), u8(list(cm[:-1])), u32([1, bad]), 2, 0, None, 0, None, BLINDING_WIRE[:1], None,
                       np.zeros((2, 4), np.uint64), np.zeros(2, np.uint32)])
    with rig.refuses(RuntimeError, "one index per proof"):
        bv.scan_serialized_mixed(raw, cm, MS, index=[1, 2, 3])
    with rig.refuses(RuntimeError, "scan_serialized_mixed: one candidate amount per proof"):
        bv.scan_serialized_mixed(raw, cm, MS, amounts=[1, 2, 3])
    with rig.refuses(RuntimeError, "blinding: 5 + 2 k_i scalars per proof (%d in all), got %d"
                     % (len(BLINDING_WIRE), len(BLINDING_WIRE) + 1)):
        bv.scan_serialized_mixed(raw, cm, MS, blinding=BLINDING + [[1]])
    with rig.refuses(ValueError, "blind_key: 32 bytes"):
        bv.scan_serialized_mixed(raw, cm, MS, blind_key=bytes(31))


# ---- the forms that take view keys ----
def test_scan_serialized_mixed_keys(rig):
    bv, name = rig.bv, "bpp_range_scan_serialized_mixed_keys"
    masks = [[5, 1 << 255 | 9, 0, (1 << 64) + 1], [1, 2, 3, 4]]
    rig.rec.writes[name] = {11: [w for row in masks for x in row for w in limbs(x)], 12: [0, 3, 2, 1, 1, 1, 0, 3]}
    m0, s0 = np.zeros((2, COUNT, 4), np.uint64), np.zeros((2, COUNT), np.uint32)
    amounts = [[1, 2, 3, 4], [5, 6, 7, 1 << 63]]
    for kw, flags in flag_cases("transcript", "uncompressed", "amount64"):
        unc = kw["uncompressed"]
        raw, cm = rig.stream(MS, unc), rig.commitments(MS, unc)
        head = [H, u8(list(raw)), u8(list(cm)), u32(MS), COUNT, flags]
        for ms in (MS, None):
            status, got = bv.scan_serialized_mixed_keys(raw, cm, ms, KEYS, **kw)
            rig.one(name, head + [packed_keys(), 2, 0, None, None, m0, s0])
            assert status.dtype == np.uint32 and status.tolist() == [[0, 3, 2, 1], [1, 1, 0, 3]] and got == masks
        bv.scan_serialized_mixed_keys(raw, cm, MS, [bytearray(k) for k in KEYS], index_base=1 << 63, index=range(4),
                                      amounts=amounts, **kw)
        rig.one(name, head + [packed_keys(), 2, 1 << 63, u64([0, 1, 2, 3]), u64([1, 2, 3, 4, 5, 6, 7, 1 << 63]), m0, s0])
        with rig.refuses(RuntimeError, "scan_serialized_mixed_keys: %d bytes of proofs, the shapes in ms need %d"
                         % (len(raw) - 1, len(raw))):
            bv.scan_serialized_mixed_keys(raw[:-1], cm, MS, KEYS, **kw)
        with rig.refuses(RuntimeError, "scan_serialized_mixed_keys: ms[i] commitments per proof"):
            bv.scan_serialized_mixed_keys(raw, cm[:-1], None, KEYS, **kw)
    raw, cm = rig.stream(MS, False), rig.commitments(MS, False)
    # the transcript is on unless the caller says otherwise
    bv.scan_serialized_mixed_keys(raw, cm, MS, KEYS)
    rig.one(name, [H, u8(list(raw)), u8(list(cm)), u32(MS), COUNT, 1, packed_keys(), 2, 0, None, None, m0, s0])
    # no keys; no proofs
    status, got = bv.scan_serialized_mixed_keys(raw, cm, MS, [], index=range(4), amounts=[])
    rig.one(name, [H, u8(list(raw)), u8(list(cm)), u32(MS), COUNT, 1, None, 0, 0, u64([0, 1, 2, 3]), None, None, None])
    assert status.shape == (0, COUNT) and got == []
    for ms in ([], None):
        status, got = bv.scan_serialized_mixed_keys(b"", b"", ms, KEYS, amounts=[[], []])
        rig.one(name, [H, None, None, None, 0, 1, packed_keys(), 2, 0, None, None, None, None])
        assert status.shape == (2, 0) and got == [[], []]
    for bad in (3, 8, 0):
        bv.scan_serialized_mixed_keys(raw[:-1], cm[:-1], [1, bad], KEYS)
        rig.one(name, [H, u8(list(raw[:-1])), u8(list(cm[:-1])), u32([1, bad]), 2, 1, packed_keys(), 2, 0, None, None,
                       np.zeros((2, 2, 4), np.uint64), np.zeros((2, 2), np.uint32)])
    with rig.refuses(RuntimeError, "scan_serialized_mixed_keys: every key is 32 bytes"):
        bv.scan_serialized_mixed_keys(raw, cm, MS, [KEYS[0], KEYS[1][:31]])
    with rig.refuses(RuntimeError, "scan_serialized_mixed_keys: one blinding index per proof"):
        bv.scan_serialized_mixed_keys(raw, cm, MS, KEYS, index=[1, 2, 3])
    with rig.refuses(RuntimeError, "scan_serialized_mixed_keys: K x count candidate amounts"):
        bv.scan_serialized_mixed_keys(raw, cm, MS, KEYS, amounts=[[1, 2, 3], [5, 6, 7]])


def test_verify_find_serialized_mixed_keys(rig):
    bv = rig.bv
    plain, tagged = "bpp_range_verify_find_serialized_mixed_keys", "bpp_range_verify_find_tagged_serialized_mixed_keys"
    rig.rec.writes[plain] = {11: [0, 1, 2, 0], 12: HIT_WORDS, 14: [2]}
    rig.rec.writes[tagged] = {11: [0, 1, 2, 0], 12: HIT_WORDS, 14: [2], 16: [3]}
    ok0, one0 = np.zeros(COUNT, np.uint32), np.zeros(1, np.uint32)
    cand = [[1, 2, 3, 4], [5, 6, 7, 1 << 63]]
    tags = [9, 8, 7, 255]
    for kw, flags in flag_cases("uncompressed", "amount64", "sealed"):
        unc = kw["uncompressed"]
        raw, cm = rig.stream(MS, unc), rig.commitments(MS, unc)
        amounts, am = ([4, 3, 2, 1 << 63], u64([4, 3, 2, 1 << 63])) if kw["sealed"] else (cand, u64(cand).reshape(-1))
        head = [H, u8(list(raw)), u8(list(cm)), u32(MS), COUNT, flags | 1, packed_keys(), 2]   # the transcript bit is forced
        for ms in (MS, None):
            res = bv.verify_find_serialized_mixed_keys(raw, cm, ms, KEYS, amounts, **kw)
            rig.one(plain, head + [0, None, am, ok0, np.zeros((8, 12), np.uint32), 8, one0])
            assert len(res) == 3 and res[0].dtype == np.uint32 and res[0].tolist() == [0, 1, 2, 0] and res[1:] == (HITS, 2)
        for tg in (tags, bytes(tags), bytearray(tags), u8(tags)):
            res = bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, amounts, index_base=1 << 63, index=range(4), max_hits=5,
                                                       tags=tg, **kw)
            rig.one(tagged, head + [1 << 63, u64([0, 1, 2, 3]), am, ok0, np.zeros((5, 12), np.uint32), 5, one0, u8(tags), one0])
            assert len(res) == 4 and res[0].tolist() == [0, 1, 2, 0] and res[1:] == (HITS, 2, 3)
        # tags = 0 is the untagged entry, like None
        res = bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, amounts, max_hits=5, tags=0, **kw)
        rig.one(plain, head + [0, None, am, ok0, np.zeros((5, 12), np.uint32), 5, one0])
        assert len(res) == 3
        with rig.refuses(RuntimeError, "verify_find_serialized_mixed_keys: %d bytes of proofs, the shapes in ms need %d"
                         % (len(raw) - 1, len(raw))):
            bv.verify_find_serialized_mixed_keys(raw[:-1], cm, MS, KEYS, amounts, **kw)
        with rig.refuses(RuntimeError, "verify_find_serialized_mixed_keys: ms[i] commitments per proof"):
            bv.verify_find_serialized_mixed_keys(raw, cm[:-1], None, KEYS, amounts, **kw)
    raw, cm = rig.stream(MS, False), rig.commitments(MS, False)
    rk, rc = u8(list(raw)), u8(list(cm))
    # more hits than room: found is reported, the list holds what was written
    rig.rec.writes[plain][14] = rig.rec.writes[tagged][14] = [7]
    ok, hits, found = bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, cand, max_hits=1)
    rig.one(plain, [H, rk, rc, u32(MS), COUNT, 1, packed_keys(), 2, 0, None, u64(cand).reshape(-1), ok0,
                    np.zeros((1, 12), np.uint32), 1, one0])
    assert found == 7 and hits == HITS[:1]
    ok, hits, found, cands = bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, cand, max_hits=0, tags=tags)
    rig.one(tagged, [H, rk, rc, u32(MS), COUNT, 1, packed_keys(), 2, 0, None, u64(cand).reshape(-1), ok0, None, 0, one0,
                     u8(tags), one0])
    assert found == 7 and hits == [] and cands == 3
    rig.rec.writes[plain][14] = rig.rec.writes[tagged][14] = [0]
    # no keys: still a verification; no proofs
    res = bv.verify_find_serialized_mixed_keys(raw, cm, MS)
    rig.one(plain, [H, rk, rc, u32(MS), COUNT, 1, None, 0, 0, None, None, ok0, None, 0, one0])
    assert res[1:] == ([], 0)
    res = bv.verify_find_serialized_mixed_keys(raw, cm, MS, [], [], sealed=False, tags=tags)
    rig.one(tagged, [H, rk, rc, u32(MS), COUNT, 1, None, 0, 0, None, None, ok0, None, 0, one0, None, one0])
    assert res[1:] == ([], 0, 3)
    for ms in ([], None):
        res = bv.verify_find_serialized_mixed_keys(b"", b"", ms, KEYS, [[], []], tags=b"")
        rig.one(tagged, [H, None, None, None, 0, 1, packed_keys(), 2, 0, None, None, None, None, 0, one0, None, one0])
        assert res[0].shape == (0,)
    for bad in (3, 8, 0):
        bv.verify_find_serialized_mixed_keys(raw[:-1], cm[:-1], [1, bad], KEYS, [1, 2], sealed=True)
        rig.one(plain, [H, rk[:-1], rc[:-1], u32([1, bad]), 2, 1 | SEALED, packed_keys(), 2, 0, None, u64([1, 2]),
                        np.zeros(2, np.uint32), np.zeros((4, 12), np.uint32), 4, one0])
    with rig.refuses(RuntimeError, "verify_find_serialized_mixed_keys: every key is 32 bytes"):
        bv.verify_find_serialized_mixed_keys(raw, cm, MS, [KEYS[0][:31]], [[1, 2, 3, 4]])
    with rig.refuses(RuntimeError, "verify_find_serialized_mixed_keys: one blinding index per proof"):
        bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, cand, index=[1, 2, 3])
    with rig.refuses(RuntimeError, "verify_find_serialized_mixed_keys: one sealed amount per proof"):
        bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, [1, 2, 3], sealed=True)
    with rig.refuses(RuntimeError, "verify_find_serialized_mixed_keys: K x count candidate amounts"):
        bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, [[1, 2, 3], [5, 6, 7]])
    with rig.refuses(RuntimeError, "verify_find_serialized_mixed_keys: one view tag per proof"):
        bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, cand, tags=tags[:3])


def test_verify_find_outputs_serialized_mixed_keys(rig):
    bv, name = rig.bv, "bpp_range_verify_find_outputs_serialized_mixed_keys"
    rig.rec.writes[name] = {12: [0, 1, 2, 0], 13: HIT_WORDS, 15: [2], 16: [3]}
    ok0, one0 = np.zeros(COUNT, np.uint32), np.zeros(1, np.uint32)
    sealed = [10, 11, 12, 13, 14, 15, 16, 1 << 63]
    tags = [9, 8, 7, 6, 5, 4, 3, 255]
    for kw, flags in flag_cases("uncompressed", "amount64"):
        unc = kw["uncompressed"]
        raw, cm = rig.stream(MS, unc), rig.commitments(MS, unc)
        head = [H, u8(list(raw)), u8(list(cm)), u32(MS), COUNT, flags | 1, packed_keys(), 2]
        for ms in (MS, None):
            res = bv.verify_find_outputs_serialized_mixed_keys(raw, cm, ms, KEYS, sealed, tags, **kw)
            rig.one(name, head + [0, None, u64(sealed), u8(tags), ok0, np.zeros((2 * N_OUT, 12), np.uint32), 2 * N_OUT, one0, one0])
            assert len(res) == 4 and res[0].dtype == np.uint32 and res[0].tolist() == [0, 1, 2, 0] and res[1:] == (HITS, 2, 3)
        for tg in (bytes(tags), u8(tags)):
            bv.verify_find_outputs_serialized_mixed_keys(raw, cm, MS, KEYS, u64(sealed), tg, index_base=1 << 63, index=range(4),
                                                         max_hits=3, **kw)
            rig.one(name, head + [1 << 63, u64([0, 1, 2, 3]), u64(sealed), u8(tags), ok0, np.zeros((3, 12), np.uint32), 3,
                                  one0, one0])
        with rig.refuses(RuntimeError, "verify_find_outputs_serialized_mixed_keys: %d bytes of proofs, the shapes in ms need %d"
                         % (len(raw) - 1, len(raw))):
            bv.verify_find_outputs_serialized_mixed_keys(raw[:-1], cm, MS, KEYS, sealed, tags, **kw)
        with rig.refuses(RuntimeError, "verify_find_outputs_serialized_mixed_keys: ms[i] commitments per proof"):
            bv.verify_find_outputs_serialized_mixed_keys(raw, cm[:-1], None, KEYS, sealed, tags, **kw)
    raw, cm = rig.stream(MS, False), rig.commitments(MS, False)
    rk, rc = u8(list(raw)), u8(list(cm))
    rig.rec.writes[name][15] = [7]
    ok, hits, found, cands = bv.verify_find_outputs_serialized_mixed_keys(raw, cm, MS, KEYS, sealed, tags, max_hits=1)
    rig.one(name, [H, rk, rc, u32(MS), COUNT, 1, packed_keys(), 2, 0, None, u64(sealed), u8(tags), ok0,
                   np.zeros((1, 12), np.uint32), 1, one0, one0])
    assert found == 7 and hits == HITS[:1] and cands == 3
    rig.rec.writes[name][15] = [0]
    # no keys: still a verification, sealed and tags are not looked at; no proofs
    res = bv.verify_find_outputs_serialized_mixed_keys(raw, cm, MS)
    rig.one(name, [H, rk, rc, u32(MS), COUNT, 1, None, 0, 0, None, None, None, ok0, None, 0, one0, one0])
    assert res[1:] == ([], 0, 3)
    for ms in ([], None):
        res = bv.verify_find_outputs_serialized_mixed_keys(b"", b"", ms, KEYS)
        rig.one(name, [H, None, None, None, 0, 1, packed_keys(), 2, 0, None, None, None, None, None, 0, one0, one0])
        assert res[0].shape == (0,)
    for bad in (3, 8, 0):
        s, t = list(range(20, 21 + bad)), list(range(1 + bad))
        bv.verify_find_outputs_serialized_mixed_keys(raw[:-1], cm[:-1], [1, bad], KEYS, s, t)
        rig.one(name, [H, rk[:-1], rc[:-1], u32([1, bad]), 2, 1, packed_keys(), 2, 0, None, u64(s), u8(t),
                       np.zeros(2, np.uint32), np.zeros((2 * (1 + bad), 12), np.uint32), 2 * (1 + bad), one0, one0])
    with rig.refuses(RuntimeError, "verify_find_outputs_serialized_mixed_keys: every key is 32 bytes"):
        bv.verify_find_outputs_serialized_mixed_keys(raw, cm, MS, [KEYS[0][:31]], sealed, tags)
    with rig.refuses(RuntimeError, "verify_find_outputs_serialized_mixed_keys: one blinding index per proof"):
        bv.verify_find_outputs_serialized_mixed_keys(raw, cm, MS, KEYS, sealed, tags, index=[1, 2, 3])
    with rig.refuses(RuntimeError, "verify_find_outputs_serialized_mixed_keys: one sealed amount and one tag per output"):
        bv.verify_find_outputs_serialized_mixed_keys(raw, cm, MS, KEYS, sealed[:-1], tags)
    with rig.refuses(RuntimeError, "verify_find_outputs_serialized_mixed_keys: one sealed amount and one tag per output"):
        bv.verify_find_outputs_serialized_mixed_keys(raw, cm, MS, KEYS, sealed, tags[:-1])


def test_make_outputs(rig):
    bv, name = rig.bv, "bpp_outputs_make"
    keys = [bytes([i]) * 32 for i in range(N_OUT)]
    kb = u8([i for i in range(N_OUT) for _ in range(32)])
    amounts = [1, 2, 3, 4, 5, 6, 7, 1 << 63]
    j = u32([0, 0, 1, 0, 1, 2, 3, 0])
    rig.rec.writes[name] = {6: list(range(4 * N_OUT)), 7: list(range(50, 50 + N_OUT)), 8: list(range(200, 200 + N_OUT))}
    outs = [np.zeros((N_OUT, 4), np.uint64), np.zeros(N_OUT, np.uint64), np.zeros(N_OUT, np.uint8)]
    masks, sealed, tags = bv.make_outputs(keys, amounts, MS, index_base=(1 << 63) + 5)
    base = (1 << 63) + 5
    rig.one(name, [AH, kb, u64([base, base + 1, base + 1, base + 2, base + 2, base + 2, base + 2, base + 3]), j, u64(amounts), N_OUT] + outs)
    assert masks.tolist() == np.arange(4 * N_OUT).reshape(N_OUT, 4).tolist() and masks.dtype == np.uint64
    assert sealed.tolist() == list(range(50, 50 + N_OUT)) and sealed.dtype == np.uint64
    assert tags.tolist() == list(range(200, 200 + N_OUT)) and tags.dtype == np.uint8
    bv.make_outputs([bytearray(k) for k in keys], u64(amounts), u32(MS), index_base=9, index=[40, 30, 1 << 63, 10])
    rig.one(name, [AH, kb, u64([40, 30, 30, 1 << 63, 1 << 63, 1 << 63, 1 << 63, 10]), j, u64(amounts), N_OUT] + outs)
    # shapes the verifier does not take are none of this call's business
    bv.make_outputs(keys[:4], amounts[:4], [3, 0, 1])
    rig.one(name, [AH, kb[:128], u64([0, 0, 0, 2]), u32([0, 1, 2, 0]), u64(amounts[:4]), 4,
                   np.zeros((4, 4), np.uint64), np.zeros(4, np.uint64), np.zeros(4, np.uint8)])
    # no outputs: no call
    masks, sealed, tags = bv.make_outputs([], [], [])
    assert rig.rec.calls == [] and masks.shape == (0, 4) and sealed.shape == (0,) and tags.shape == (0,)
    with rig.refuses(RuntimeError, "make_outputs: every key is 32 bytes"):
        bv.make_outputs(keys[:-1] + [keys[-1][:31]], amounts, MS)
    with rig.refuses(RuntimeError, "make_outputs: one key and one amount per output, sum(ms) of them"):
        bv.make_outputs(keys[:-1], amounts, MS)
    with rig.refuses(RuntimeError, "make_outputs: one key and one amount per output, sum(ms) of them"):
        bv.make_outputs(keys, amounts[:-1], MS)
    with rig.refuses(RuntimeError, "make_outputs: one blinding index per proof"):
        bv.make_outputs(keys, amounts, MS, index=[1, 2, 3])


def _key_forms(rig):
    """(entry, position of the packed keys, the call) for the four forms that pack view keys"""
    bv = rig.bv
    raw, cm = rig.stream(MS, False), rig.commitments(MS, False)
    cand = [[1, 2, 3, 4], [5, 6, 7, 8]]
    keys8 = [bytes([i + 1]) * 32 for i in range(N_OUT)]
    return [
        ("bpp_range_scan_serialized_mixed_keys", 6, lambda: bv.scan_serialized_mixed_keys(raw, cm, MS, KEYS)),
        ("bpp_range_verify_find_serialized_mixed_keys", 6, lambda: bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, cand)),
        ("bpp_range_verify_find_tagged_serialized_mixed_keys", 6,
         lambda: bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, cand, tags=[1, 2, 3, 4])),
        ("bpp_range_verify_find_outputs_serialized_mixed_keys", 6,
         lambda: bv.verify_find_outputs_serialized_mixed_keys(raw, cm, MS, KEYS, range(N_OUT), bytes(N_OUT))),
        ("bpp_outputs_make", 1, lambda: bv.make_outputs(keys8, range(N_OUT), MS)),
    ]


def test_packed_keys_are_wiped_after_the_call(rig):
    for name, pos, call in _key_forms(rig):
        call()
        assert rig.rec.calls[-1][0] == name and rig.rec.calls[-1][1][pos].any()   # the keys were there during the call
        kb = rig.rec.live[name][pos]
        assert kb.dtype == np.uint8 and len(kb) >= 64 and not kb.any(), name


def test_packed_keys_are_wiped_when_the_library_refuses(rig):
    # the one assertion of this file that the code before the shared packed-keys helper fails: it wiped the copy only
    # after check() had passed
    for name, pos, call in _key_forms(rig):
        rig.rec.rc[name] = -1
        with pytest.raises(api.BppError) as e:
            call()
        assert e.value.code == -1 and str(e.value).startswith(name + " failed with code -1")
        assert rig.rec.calls[-1][0] == name and rig.rec.calls[-1][1][pos].any()
        kb = rig.rec.live[name][pos]
        assert kb.dtype == np.uint8 and len(kb) >= 64 and not kb.any(), name


# ---- sealed amounts and view tags ----
def test_seal_amounts(rig):
    bv, name = rig.bv, "bpp_amounts_seal"
    key = bytes(range(32))
    amounts = [1, 2, (1 << 64) - 1]
    rig.rec.writes[name] = {6: [7, 8, 1 << 63]}
    out = bv.seal_amounts(key, amounts, index_base=1 << 63)
    rig.one(name, [AH, key, 1 << 63, None, u64(amounts), 3, np.zeros(3, np.uint64)])
    assert out.dtype == np.uint64 and out.tolist() == [7, 8, 1 << 63]
    bv.seal_amounts(key, u64(amounts), index=[5, 1 << 63, 0])
    rig.one(name, [AH, key, 0, u64([5, 1 << 63, 0]), u64(amounts), 3, np.zeros(3, np.uint64)])
    assert bv.seal_amounts(key, []).shape == (0,)
    rig.one(name, [AH, key, 0, None, None, 0, None])
    bv.seal_amounts(key, [], index=[])
    rig.one(name, [AH, key, 0, u64([]), None, 0, None])
    with rig.refuses(RuntimeError, "seal_amounts: one blinding index per amount"):
        bv.seal_amounts(key, amounts, index=[1, 2])


def test_view_tags(rig):
    bv, name = rig.bv, "bpp_view_tags"
    key = bytes(range(32))
    rig.rec.writes[name] = {5: [7, 8, 255]}
    out = bv.view_tags(key, 3, index_base=1 << 63)
    rig.one(name, [AH, key, 1 << 63, None, 3, np.zeros(3, np.uint8)])
    assert out.dtype == np.uint8 and out.tolist() == [7, 8, 255]
    for count in (None, 3):
        bv.view_tags(key, count, index=[5, 1 << 63, 0])
        rig.one(name, [AH, key, 0, u64([5, 1 << 63, 0]), 3, np.zeros(3, np.uint8)])
    for kw in ({}, {"count": 0}, {"index": []}, {"count": 0, "index": []}):
        assert bv.view_tags(key, **kw).shape == (0,)
        rig.one(name, [AH, key, 0, None, 0, None])
    with rig.refuses(RuntimeError, "view_tags: one blinding index per output"):
        bv.view_tags(key, 3, index=[1, 2])


# ---- the provers ----
VALUES = [[1], [2, 3], [4, 5, 6, (1 << 64) - 1], [1 << 63]]
GAMMAS = [[11], [12, 1 << 200], [14, 15, 16, 17], [(1 << 255) + 3]]
GAMMAS_WIRE = u64([limbs(g) for row in GAMMAS for g in row])


def test_prove_batch_mixed(rig):
    bv, name, PW = rig.bv, "bpp_range_prove_batch_mixed", rig.PW
    key = bytes(range(32))
    vals = u64([x for row in VALUES for x in row])
    npts, nch = [points_of(m) for m in MS], [3 + k for k in K_OF]
    pts0, sc0, ch0 = np.zeros((sum(npts), PW), np.uint64), np.zeros((COUNT, 3, 4), np.uint64), np.zeros((sum(nch), 4), np.uint64)
    rig.rec.writes[name] = {8: list(range(sum(npts) * PW)), 9: list(range(COUNT * 12)), 10: list(range(sum(nch) * 4))}
    all_pts, all_ch = np.arange(sum(npts) * PW).reshape(-1, PW), np.arange(sum(nch) * 4).reshape(-1, 4)
    po, co = np.cumsum([0] + npts), np.cumsum([0] + nch)
    for kw, flags in flag_cases("transcript", "amount64"):
        for gammas in (GAMMAS, [[u64(limbs(g)) for g in row] for row in GAMMAS]):
            res = bv.prove_batch_mixed(VALUES, gammas, **kw)
            rig.one(name, [H, vals, GAMMAS_WIRE, u32(MS), COUNT, flags, None, 0, pts0, sc0, None])
            assert len(res) == 2 and len(res[0]) == COUNT
            for i in range(COUNT):
                assert res[0][i].dtype == np.uint64 and np.array_equal(res[0][i], all_pts[po[i]:po[i + 1]])
            assert np.array_equal(res[1], np.arange(COUNT * 12).reshape(COUNT, 3, 4))
        res = bv.prove_batch_mixed(VALUES, GAMMAS, index_base=1 << 63, challenges=True, **kw)
        rig.one(name, [H, vals, GAMMAS_WIRE, u32(MS), COUNT, flags, None, 1 << 63, pts0, sc0, ch0])
        assert len(res) == 3 and len(res[2]) == COUNT
        for i in range(COUNT):
            assert np.array_equal(res[0][i], all_pts[po[i]:po[i + 1]]) and np.array_equal(res[2][i], all_ch[co[i]:co[i + 1]])
    bv.prove_batch_mixed(VALUES, GAMMAS, transcript=True, blind_key=key, index_base=5)
    rig.one(name, [H, vals, GAMMAS_WIRE, u32(MS), COUNT, 1, key, 5, pts0, sc0, None])
    recs, sc = bv.prove_batch_mixed([], [])
    rig.one(name, [H, None, None, None, 0, 0, None, 0, np.zeros((1, PW), np.uint64), None, None])
    assert recs == [] and sc.shape == (0, 3, 4)
    for bad in (3, 8, 0):   # no sizes to cut by: room for one point, the library names the proof
        recs, sc = bv.prove_batch_mixed([[1], [2] * bad], [[3], [4] * bad])
        rig.one(name, [H, u64([1] + [2] * bad), u64([limbs(3)] + [limbs(4)] * bad), u32([1, bad]), 2, 0, None, 0,
                       np.zeros((1, PW), np.uint64), np.zeros((2, 3, 4), np.uint64), None])
        assert [r.shape for r in recs] == [(0, PW), (0, PW)]
    with rig.refuses(RuntimeError, "one gamma per value"):
        bv.prove_batch_mixed(VALUES, GAMMAS[:3])
    with rig.refuses(RuntimeError, "one gamma per value"):
        bv.prove_batch_mixed(VALUES, GAMMAS[:3] + [[1, 2]])
    with rig.refuses(ValueError, "blind_key: 32 bytes, transcript mode only"):
        bv.prove_batch_mixed(VALUES, GAMMAS, transcript=True, blind_key=bytes(31))
    with rig.refuses(ValueError, "blind_key: 32 bytes, transcript mode only"):
        bv.prove_batch_mixed(VALUES, GAMMAS, blind_key=key)


def test_prove_serialized_mixed(rig):
    bv, name = rig.bv, "bpp_range_prove_batch_serialized_mixed"
    key = bytes(range(32))
    vals = u64([x for row in VALUES for x in row])
    for kw, flags in flag_cases("transcript", "uncompressed", "amount64"):
        unc = kw["uncompressed"]
        nbytes, cbytes = sum(rig.proof_bytes(m, unc) for m in MS), N_OUT * rig.point_bytes(unc)
        rig.rec.writes[name] = {8: [i % 251 for i in range(nbytes)], 9: [i % 241 for i in range(cbytes)]}
        proofs, cm, ms = bv.prove_serialized_mixed(VALUES, GAMMAS, index_base=1 << 63, **kw)
        rig.one(name, [H, vals, GAMMAS_WIRE, u32(MS), COUNT, flags, None, 1 << 63, np.zeros(nbytes, np.uint8), np.zeros(cbytes, np.uint8)])
        assert type(proofs) is bytes and proofs == bytes(i % 251 for i in range(nbytes))
        assert type(cm) is bytes and cm == bytes(i % 241 for i in range(cbytes))
        assert ms.dtype == np.uint32 and ms.tolist() == MS
    bv.prove_serialized_mixed(VALUES, GAMMAS, transcript=True, blind_key=key)
    nbytes, cbytes = sum(rig.proof_bytes(m, False) for m in MS), N_OUT * rig.point_bytes(False)
    rig.one(name, [H, vals, GAMMAS_WIRE, u32(MS), COUNT, 1, key, 0, np.zeros(nbytes, np.uint8), np.zeros(cbytes, np.uint8)])
    proofs, cm, ms = bv.prove_serialized_mixed([], [])
    rig.one(name, [H, None, None, None, 0, 0, None, 0, np.zeros(1, np.uint8), np.zeros(1, np.uint8)])
    assert proofs == b"" and cm == b"" and len(ms) == 0
    for bad in (3, 8, 0):
        proofs, cm, ms = bv.prove_serialized_mixed([[1], [2] * bad], [[3], [4] * bad])
        rig.one(name, [H, u64([1] + [2] * bad), u64([limbs(3)] + [limbs(4)] * bad), u32([1, bad]), 2, 0, None, 0,
                       np.zeros(1, np.uint8), np.zeros((1 + bad) * rig.point_bytes(False), np.uint8)])
        assert proofs == b""
    with rig.refuses(RuntimeError, "one gamma per value"):
        bv.prove_serialized_mixed(VALUES, GAMMAS[:3])
    with rig.refuses(ValueError, "blind_key: 32 bytes, transcript mode only"):
        bv.prove_serialized_mixed(VALUES, GAMMAS, transcript=True, blind_key=bytes(31))
    with rig.refuses(ValueError, "blind_key: 32 bytes, transcript mode only"):
        bv.prove_serialized_mixed(VALUES, GAMMAS, blind_key=key)


# ---- the *_device one-liners: device addresses go through as given, 0 as None ----
def test_verify_serialized_mixed_device(rig):
    bv, name = rig.bv, "bpp_range_verify_batch_serialized_mixed_device"
    for kw, flags in flag_cases("transcript", "uncompressed"):
        bv.verify_serialized_mixed_device(11, 12, MS, 13, 14, 15, **kw)
        rig.one(name, [H, 11, 12, u32(MS), COUNT, flags, 13, 14, 15, None])
    bv.verify_serialized_mixed_device(11, 12, [], 13, 14, 15, stream=16)   # this one hands an empty ms over as an array
    rig.one(name, [H, 11, 12, u32([]), 0, 0, 13, 14, 15, 16])


def test_scan_serialized_mixed_device(rig):
    bv, name = rig.bv, "bpp_range_scan_serialized_mixed_device"
    key = bytes(range(32))
    for kw, flags in flag_cases("transcript", "uncompressed", "amount64"):
        bv.scan_serialized_mixed_device(11, 12, MS, 13, 14, 15, 16, **kw)
        rig.one(name, [H, 11, 12, u32(MS), COUNT, flags, None, 0, None, None, None, 13, 14, 15, 16, None])
    bv.scan_serialized_mixed_device(11, 12, [], 13, 14, 15, 16, stream=17, blind_key=key, index_base=1 << 63, d_index=18,
                                    d_blinding=19, d_amounts=20)
    rig.one(name, [H, 11, 12, None, 0, 0, key, 1 << 63, 18, 19, 20, 13, 14, 15, 16, 17])


def test_scan_serialized_mixed_keys_device(rig):
    bv, name = rig.bv, "bpp_range_scan_serialized_mixed_keys_device"
    for kw, flags in flag_cases("transcript", "uncompressed", "amount64"):
        bv.scan_serialized_mixed_keys_device(11, 12, MS, 13, 2, 14, 15, 16, 17, **kw)
        rig.one(name, [H, 11, 12, u32(MS), COUNT, flags, 13, 2, 0, None, None, 14, 15, 16, 17, None])
    bv.scan_serialized_mixed_keys_device(11, 12, [], 0, 0, 14, 15, 16, 17, stream=18, index_base=1 << 63, d_index=19, d_amounts=20)
    rig.one(name, [H, 11, 12, None, 0, 1, None, 0, 1 << 63, 19, 20, 14, 15, 16, 17, 18])


def test_verify_find_serialized_mixed_keys_device(rig):
    bv = rig.bv
    plain, tagged = "bpp_range_verify_find_serialized_mixed_keys_device", "bpp_range_verify_find_tagged_serialized_mixed_keys_device"
    for kw, flags in flag_cases("uncompressed", "amount64", "sealed"):
        bv.verify_find_serialized_mixed_keys_device(11, 12, MS, 13, 2, 14, 15, 16, 8, 17, 18, 19, **kw)
        rig.one(plain, [H, 11, 12, u32(MS), COUNT, flags | 1, 13, 2, 0, None, 14, 15, 16, 8, 17, 18, 19, None])
        bv.verify_find_serialized_mixed_keys_device(11, 12, MS, 13, 2, 14, 15, 16, 8, 17, 18, 19, d_tags=20, **kw)
        rig.one(tagged, [H, 11, 12, u32(MS), COUNT, flags | 1, 13, 2, 0, None, 14, 15, 16, 8, 17, 20, None, 18, 19, None])
    bv.verify_find_serialized_mixed_keys_device(11, 12, [], 0, 0, 0, 0, 0, 0, 0, 18, 19, stream=21, index_base=1 << 63, d_index=22,
                                                d_n_candidates=23)
    rig.one(plain, [H, 11, 12, None, 0, 1, None, 0, 1 << 63, 22, None, None, None, 0, None, 18, 19, 21])
    bv.verify_find_serialized_mixed_keys_device(11, 12, [], 0, 0, 0, 0, 0, 0, 0, 18, 19, stream=21, index_base=1 << 63, d_index=22,
                                                d_tags=20, d_n_candidates=23)
    rig.one(tagged, [H, 11, 12, None, 0, 1, None, 0, 1 << 63, 22, None, None, None, 0, None, 20, 23, 18, 19, 21])


def test_verify_find_outputs_serialized_mixed_keys_device(rig):
    bv, name = rig.bv, "bpp_range_verify_find_outputs_serialized_mixed_keys_device"
    for kw, flags in flag_cases("uncompressed", "amount64"):
        bv.verify_find_outputs_serialized_mixed_keys_device(11, 12, MS, 13, 2, 14, 15, 16, 17, 8, 18, 19, 20, **kw)
        rig.one(name, [H, 11, 12, u32(MS), COUNT, flags | 1, 13, 2, 0, None, 14, 15, 16, 17, 8, 18, None, 19, 20, None])
    bv.verify_find_outputs_serialized_mixed_keys_device(11, 12, [], 0, 0, 0, 0, 0, 0, 0, 0, 19, 20, stream=21, index_base=1 << 63,
                                                        d_index=22, d_n_candidates=23)
    rig.one(name, [H, 11, 12, None, 0, 1, None, 0, 1 << 63, 22, None, None, None, None, 0, None, 23, 19, 20, 21])


def test_recover_masks_device(rig):
    bv, name = rig.bv, "bpp_range_recover_masks_mixed_device"
    key = bytes(range(32))
    bv.recover_masks_device(11, MS, 12, 13, 14)
    rig.one(name, [H, 11, u32(MS), COUNT, None, None, 0, None, None, 12, 13, 14, None])
    bv.recover_masks_device(11, [], 12, 13, 14, stream=15, d_challenges=16, blind_key=key, index_base=1 << 63, d_index=17,
                            d_blinding=18)
    rig.one(name, [H, 11, None, 0, 16, key, 1 << 63, 17, 18, 12, 13, 14, 15])


def test_prove_mixed_device(rig):
    bv, name = rig.bv, "bpp_range_prove_batch_mixed_device"
    key = bytes(range(32))
    for kw, flags in flag_cases("transcript", "amount64"):
        bv.prove_mixed_device(11, 12, MS, 13, 14, 15, 16, **kw)
        rig.one(name, [H, 11, 12, u32(MS), COUNT, flags, None, 0, None, 13, 14, None, 15, 16, None])
    bv.prove_mixed_device(11, 12, [], 13, 14, 15, 16, stream=17, transcript=True, d_out_challenges=18, blind_key=key,
                          index_base=1 << 63, d_blinding=19)
    rig.one(name, [H, 11, 12, None, 0, 1, key, 1 << 63, 19, 13, 14, 18, 15, 16, 17])


def test_prove_serialized_mixed_device(rig):
    bv, name = rig.bv, "bpp_range_prove_batch_serialized_mixed_device"
    key = bytes(range(32))
    for kw, flags in flag_cases("transcript", "uncompressed", "amount64"):
        bv.prove_serialized_mixed_device(11, 12, MS, 13, 14, 15, 16, **kw)
        rig.one(name, [H, 11, 12, u32(MS), COUNT, flags, None, 0, None, 13, 14, 15, 16, None])
    bv.prove_serialized_mixed_device(11, 12, [], 13, 14, 15, 16, stream=17, transcript=True, blind_key=key, index_base=1 << 63,
                                     d_blinding=19)
    rig.one(name, [H, 11, 12, None, 0, 1, key, 1 << 63, 19, 13, 14, 15, 16, 17])


# ---- the shape arithmetic both classes share ----
def test_shape_helpers(rig):
    for m in (1, 2, 4):
        assert rig.bv.mixed_points(m) == points_of(m)
    got = rig.bv._ms([1, 2, 4])
    assert got.dtype == np.uint32 and got.tolist() == [1, 2, 4] and got.flags["C_CONTIGUOUS"]
    assert rig.bv._ms(u64([[1, 2], [4, 1]])).tolist() == [1, 2, 4, 1]
    assert rig.rec.calls == []
