"""-m gpu: the verifier pool (include/bpp_amd.h "verifier pool") -- one batch sharded over several shards in one process,
here all on device 0: devices = (0,), (0, 0) and (0, 0, 0).

The pool adds no arithmetic, so every check is an equality: with the statuses / verdicts of the adversarial corpus
(tests/verdict_corpus.py, oracle-derived) and, word for word, with a plain BatchVerifier of the same key over the whole
batch -- for bytes through the exact and the grouped check, for wire records, for the combined check with its one reduce,
and at the edges (an empty shard, an empty batch, a bad m_of, a device that does not exist, two pools, create / destroy).
Capacity (8, 4) at window 5, the shapes of tests/test_gpu_serialized_mixed.py."""

import ctypes
import functools
import os

import numpy as np
import pytest

import verdict_corpus as VC
from gpu_util import need_gpu
from test_gpu_mixed import _raw_expect, _record
from test_gpu_serialized_mixed import CAP, CLASSES, CURVES, N, WB, _corpora, _interleave, _u8

pytestmark = pytest.mark.gpu

WORLDS = (1, 2, 3)
GROUP = 4


def _spread(cases, value):
    """the cases of one class reordered so that those with value 0 and the others alternate in proportion (the corpus
    lists its valid cases first; a contiguous cut of that order would give a shard nothing but failures)"""
    z = [c for c in cases if value(c) == 0]
    nz = [c for c in cases if value(c) != 0]
    out, i, j = [], 0, 0
    while i < len(z) or j < len(nz):
        if j >= len(nz) or (i < len(z) and i * len(nz) <= j * len(z)):
            out.append(z[i])
            i += 1
        else:
            out.append(nz[j])
            j += 1
    return out


def _py_cuts(ms, world):
    """the cut rule of include/bpp_amd.h restated (the conditions below are computed without the library)"""
    total, out, r, prefix = sum(ms), [0], 1, 0
    for i, m in enumerate(ms):
        while r < world and world * prefix >= r * total:
            out.append(i)
            r += 1
        prefix += m
    return out + [len(ms)] * (world + 1 - len(out))


@functools.lru_cache(maxsize=None)
def _byte_plan(cname):
    """-> (corpora, cases per class, sequence of (m, case index), m per proof, wanted statuses) of the bytes tests, with
    the conditions the tests rest on asserted here, before anything runs on the device"""
    cps = _corpora(cname)
    cases = {}
    for m in CLASSES:
        have = [c for c in cps[m].cases if c.status is not None]
        left_out = len(cps[m].cases) - len(have)
        assert len(have) >= 24 and left_out <= 5, (cname, m, len(have), left_out)
        cases[m] = _spread(have, lambda c: c.status)
    seq = _interleave(cases, (1, 2, 4))
    ms = [m for m, _ in seq]
    want = [cases[m][i].status for m, i in seq]
    starts_on_failure = False
    for world in (2, 3):
        cuts = _py_cuts(ms, world)
        for r in range(world):
            part = want[cuts[r]:cuts[r + 1]]
            assert 0 in part and any(part), (cname, world, r, part)
            starts_on_failure |= r > 0 and want[cuts[r]] != 0
    assert starts_on_failure, (cname, "no shard starts on a case that fails")
    return cps, cases, seq, ms, want


def _pk(B, a, cp):
    return B.PublicKey.from_points(a, cp.gh, cp.G, cp.H)


def _pool(B, a, cp, world):
    return B.VerifierPool(_pk(B, a, cp), N, CAP, window_bits=WB, devices=(0,) * world)


def test_cut_restated_equals_the_library():
    need_gpu()
    import bulletproofsplus_amd as B
    rng = np.random.default_rng(11)
    for world in range(1, 8):
        ms = (1 << rng.integers(0, 5, size=int(rng.integers(0, 60)))).tolist()
        assert B.shard_cuts(ms, len(ms), world).tolist() == _py_cuts(ms, world)


@pytest.mark.parametrize("cname", CURVES)
def test_pool_bytes_exact(cname):
    need_gpu()
    import bulletproofsplus_amd as B
    cps, cases, seq, ms, want = _byte_plan(cname)
    a = B.Arith(cname)
    bv = B.BatchVerifier(_pk(B, a, cps[CAP]), N, CAP, window_bits=WB)
    for version in ((1, 2) if cname != "ed25519" else (1,)):
        unc = version == 2
        enc = {m: [VC.encode_case(cps[m], c, version) for c in cases[m]] for m in CLASSES}
        raw, cm = _u8([enc[m][i][0] for m, i in seq]), _u8([enc[m][i][1] for m, i in seq])
        plain = bv.verify_serialized_mixed(raw, cm, ms, uncompressed=unc)
        assert plain.tolist() == want, version
        for world in WORLDS:
            pool = _pool(B, a, cps[CAP], world)
            assert pool.size == world and pool.devices == [0] * world
            assert pool.cuts(ms).tolist() == _py_cuts(ms, world)
            ok = pool.verify_serialized_mixed(raw, cm, ms, uncompressed=unc)
            bad = [(j, seq[j][0], cases[seq[j][0]][seq[j][1]].name, int(ok[j]), want[j]) for j in range(len(seq)) if ok[j] != want[j]]
            assert not bad, (version, world, bad)
            assert np.array_equal(ok, plain), (version, world)
            pool.close()
    bv.close()


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_pool_bytes_exact_transcript(cname):
    need_gpu()
    import bulletproofsplus_amd as B
    cps = {m: VC.corpus(cname, N, m, transcript=True) for m in CLASSES}
    cases = {m: list(cps[m].cases) for m in CLASSES}
    status = {m: [cps[m].container_status(c) for c in cases[m]] for m in CLASSES}
    enc = {m: [VC.encode_case(cps[m], c) for c in cases[m]] for m in CLASSES}
    seq = _interleave(cases, (4, 1, 2))
    ms = [m for m, _ in seq]
    want = [status[m][i] for m, i in seq]
    assert {0, 1} <= set(want)
    raw, cm = _u8([enc[m][i][0] for m, i in seq]), _u8([enc[m][i][1] for m, i in seq])
    a = B.Arith(cname)
    bv = B.BatchVerifier(_pk(B, a, cps[CAP]), N, CAP, window_bits=WB)
    plain = bv.verify_serialized_mixed(raw, cm, ms, transcript=True)
    assert plain.tolist() == want
    for world in WORLDS:
        pool = _pool(B, a, cps[CAP], world)
        assert pool.verify_serialized_mixed(raw, cm, ms, transcript=True).tolist() == want, world
        # the transcript binds the proofs: under the literal challenges none of them verifies
        assert 0 not in pool.verify_serialized_mixed(raw, cm, ms).tolist(), world
        pool.close()
    bv.close()


@pytest.mark.parametrize("cname", CURVES)
def test_pool_bytes_grouped(cname):
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cps, cases, seq, ms, want = _byte_plan(cname)
    enc = {m: [VC.encode_case(cps[m], c) for c in cases[m]] for m in CLASSES}
    blobs, comms = [enc[m][i][0] for m, i in seq], [enc[m][i][1] for m, i in seq]
    raw, cm = _u8(blobs), _u8(comms)
    a = B.Arith(cname)
    key, base = os.urandom(32), 1 << 40
    dev = torch.device("cuda:0")
    for world in WORLDS:
        pool = _pool(B, a, cps[CAP], world)
        ok, stats = pool.verify_serialized_mixed(raw, cm, ms, grouped=True, weight_key=key, index_base=base, group=GROUP,
                                                 return_stats=True)
        assert ok.tolist() == want, world
        assert stats[1] >= sum(1 for s in want if s == 1), (world, stats)
        # the stats are the sum of what the shards' own grouped calls report over the slices of the cut
        cuts = pool.cuts(ms).tolist()
        total = [0, 0]
        for r in range(world):
            lo, hi = cuts[r], cuts[r + 1]
            v = pool.verifier(r)
            d_p = torch.from_numpy(_u8(blobs[lo:hi])).to(dev)
            d_c = torch.from_numpy(_u8(comms[lo:hi])).to(dev)
            d_ok = torch.full((hi - lo,), 7, dtype=torch.int32, device=dev)
            wsb = v.serialized_grouped_mixed_workspace_bytes(ms[lo:hi], GROUP)
            assert wsb > 0
            d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            st = v.verify_serialized_grouped_mixed_device(d_p.data_ptr(), d_c.data_ptr(), ms[lo:hi], d_ok.data_ptr(),
                                                          d_ws.data_ptr(), wsb, weight_key=key, index_base=base + lo,
                                                          group=GROUP, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert d_ok.cpu().tolist() == want[lo:hi], (world, r)
            total = [total[0] + st[0], total[1] + st[1]]
            v.close()   # borrowed: the pool keeps it
        assert list(stats) == total, (world, stats, total)
        # a key of the pool's own choosing gives the same statuses
        assert pool.verify_serialized_mixed(raw, cm, ms, grouped=True, group=GROUP).tolist() == want, world
        pool.close()


@functools.lru_cache(maxsize=None)
def _uniform(cname, tampered=()):
    """10 valid (8, 4) proofs of the product's own prover as (records, scalars), the proofs in `tampered` spoiled"""
    import bulletproofsplus_amd as B
    a = B.Arith(cname)
    pk = B.PublicKey.new(a, N * CAP)
    bv = B.BatchVerifier(pk, N, CAP, window_bits=WB)
    vals = [[(37 * p + j) % 256 for j in range(CAP)] for p in range(10)]
    gams = [[p + j + 1 for j in range(CAP)] for p in range(10)]
    pts, scs, V = bv.prove_batch(vals, gams)
    bv.close()
    recs = np.ascontiguousarray(np.concatenate([pts, V], axis=1))
    scs = np.ascontiguousarray(scs).copy()
    for t in tampered:
        scs[t, 2, 0] ^= np.uint64(2)
    return recs, scs


@pytest.mark.parametrize("cname", CURVES)
def test_pool_wire_records(cname):
    need_gpu()
    import bulletproofsplus_amd as B
    cps = _corpora(cname)
    cases = {m: _spread([c for c in cps[m].cases if c.k_ok], lambda c: c.expect) for m in CLASSES}
    seq = _interleave(cases, (2, 4, 1))
    recs = [_record(cases[m][i]) for m, i in seq]
    scs = np.stack([cases[m][i].sc for m, i in seq])
    ms = [m for m, _ in seq]
    a = B.Arith(cname)
    bv = B.BatchVerifier(_pk(B, a, cps[CAP]), N, CAP, window_bits=WB)
    plain = bv.verify_wire_mixed(recs, scs, ms)
    want = [_raw_expect(cps[m], cases[m][i], False) for m, i in seq]
    assert sum(1 for w in want if w == 0) >= 9 and sum(1 for w in want if w == 1) >= 9
    for world in WORLDS:
        pool = _pool(B, a, cps[CAP], world)
        ok = pool.verify_wire_mixed(recs, scs, ms)
        assert np.array_equal(ok, plain), world
        bad = [(j, seq[j], int(ok[j]), want[j]) for j in range(len(seq)) if want[j] is not None and ok[j] != want[j]]
        assert not bad, (world, bad)
        pool.close()
    bv.close()
    # a uniform batch (m_of = NULL) of 10 proofs, proof 7 tampered
    recs, scs = _uniform(cname, (7,))
    pk = B.PublicKey.new(a, N * CAP)
    bv = B.BatchVerifier(pk, N, CAP, window_bits=WB)
    exp = [0] * 7 + [1, 0, 0]
    assert bv.verify_wire(recs, scs).tolist() == exp
    for world in WORLDS:
        pool = B.VerifierPool(pk, N, CAP, window_bits=WB, devices=(0,) * world)
        assert pool.verify_wire_mixed(recs, scs).tolist() == exp, world
        assert pool.verify_wire_mixed(recs, scs, [CAP] * 10).tolist() == exp, world
        pool.close()
    bv.close()


@pytest.mark.parametrize("cname", CURVES)
def test_pool_combined(cname):
    need_gpu()
    import bulletproofsplus_amd as B
    a = B.Arith(cname)
    pk = B.PublicKey.new(a, N * CAP)
    for world in WORLDS:
        pool = B.VerifierPool(pk, N, CAP, window_bits=WB, devices=(0,) * world)
        if world == 2:
            assert pool.cuts(None, 10).tolist() == [0, 5, 10]   # proofs 2 and 7 lie in different shards
        for tampered, want in (((), 0), ((7,), 1), ((2, 7), 1)):
            recs, scs = _uniform(cname, tampered)
            assert pool.verify_combined(recs, scs) == want, (world, tampered)
            assert pool.verify_combined(recs, scs, weight_key=bytes(range(32)), index_base=1 << 33) == want, (world, tampered)
        assert pool.verify_combined(recs[:0], scs[:0]) == 0, world
        # fewer proofs than shards
        recs, scs = _uniform(cname, ())
        assert pool.verify_combined(recs[:2], scs[:2]) == 0, world
        recs, scs = _uniform(cname, (7,))
        assert pool.verify_combined(recs[6:8], scs[6:8]) == 1, world
        pool.close()


def test_pool_edges():
    torch = need_gpu()
    import bulletproofsplus_amd as B
    from bulletproofsplus_amd import _lib
    cname = "secp256k1"
    cps, cases, seq, ms, want = _byte_plan(cname)
    enc = {m: [VC.encode_case(cps[m], c) for c in cases[m]] for m in CLASSES}
    blobs, comms = [enc[m][i][0] for m, i in seq], [enc[m][i][1] for m, i in seq]
    a = B.Arith(cname)
    pk = _pk(B, a, cps[CAP])
    pool = B.VerifierPool(pk, N, CAP, window_bits=WB, devices=(0, 0, 0))
    # two proofs on three shards: the last shard is empty
    assert ms[:2] == [1, 2] and pool.cuts(ms[:2]).tolist() == [0, 1, 2, 2]
    assert pool.verify_serialized_mixed(_u8(blobs[:2]), _u8(comms[:2]), ms[:2]).tolist() == want[:2]
    j = next(t for t in range(len(want) - 1) if want[t] != want[t + 1])   # a pair with two different statuses
    assert pool.verify_serialized_mixed(_u8(blobs[j:j + 2]), _u8(comms[j:j + 2]), ms[j:j + 2], grouped=True,
                                        group=GROUP).tolist() == want[j:j + 2]
    recs, scs = _uniform(cname, (7,))
    upool = B.VerifierPool(B.PublicKey.new(a, N * CAP), N, CAP, window_bits=WB, devices=(0, 0, 0))
    assert upool.cuts(None, 2).tolist() == [0, 1, 2, 2]
    assert upool.verify_wire_mixed(recs[6:8], scs[6:8]).tolist() == [0, 1]
    # an empty batch
    assert pool.verify_serialized_mixed(b"", b"", []).tolist() == []
    assert pool.verify_serialized_mixed(b"", b"", [], grouped=True, group=GROUP, return_stats=True)[1] == (0, 0)
    assert upool.verify_wire_mixed(recs[:0], scs[:0]).tolist() == []
    assert upool.verify_wire_mixed(recs[:0], scs[:0], []).tolist() == []
    # a bad m_of[7]: BPP_E_ARG naming the caller's index, nothing written
    L = _lib.lib()
    bad_ms = np.array([CAP] * 10, dtype=np.uint32)
    bad_ms[7] = 3
    ok = np.full(10, 7, dtype=np.uint32)
    stats = np.full(2, 9, dtype=np.uint64)

    def p(x):
        return x.ctypes.data_as(ctypes.c_void_p)
    rc = L.bpp_pool_verify_mixed(upool.handle, p(recs), p(scs), p(bad_ms), 10, p(ok))
    assert rc == -1 and "m_of[7]" in L.bpp_last_error().decode(), L.bpp_last_error()
    raw, cm = _u8(blobs[:10]), _u8(comms[:10])
    for mode in (0, 1):
        rc = L.bpp_pool_verify_serialized_mixed(pool.handle, p(raw), p(cm), p(bad_ms), 10, 0, mode, bytes(32), 0, GROUP, p(ok),
                                                p(stats))
        assert rc == -1 and "m_of[7]" in L.bpp_last_error().decode(), (mode, L.bpp_last_error())
    good_ms = np.array(ms[:10], dtype=np.uint32)
    for mode, key, group in ((2, bytes(32), GROUP), (1, None, GROUP), (1, bytes(32), 3), (1, bytes(32), 0)):
        rc = L.bpp_pool_verify_serialized_mixed(pool.handle, p(raw), p(cm), p(good_ms), 10, 0, mode, key, 0, group, p(ok), p(stats))
        assert rc == -1, (mode, key, group)
    assert L.bpp_pool_verify_serialized_mixed(pool.handle, p(raw), p(cm), p(good_ms), 10, 4, 0, None, 0, 0, p(ok), None) == -1
    assert L.bpp_pool_verify_combined(upool.handle, p(recs), p(scs), 10, None, 0, p(ok)) == -1
    assert ok.tolist() == [7] * 10 and stats.tolist() == [9, 9]
    with pytest.raises(B.BppError) as ei:
        upool.verify_wire_mixed(recs, scs, bad_ms)
    assert ei.value.code == -1 and "7" in str(ei.value)
    # the shards answer for themselves
    assert [L.bpp_pool_device(pool.handle, r) for r in range(4)] == [0, 0, 0, -1]
    v = ctypes.c_void_p(1)
    assert L.bpp_pool_verifier(pool.handle, 3, ctypes.byref(v)) == -1 and not v.value
    assert pool.verifier(2).table_bytes > 0
    # a device that does not exist: BPP_E_HIP from that shard, no pool
    with pytest.raises(B.BppError) as ei:
        B.VerifierPool(pk, N, CAP, window_bits=WB, devices=(torch.cuda.device_count(),))
    assert ei.value.code == -2 and "shard 0 (device %d): " % torch.cuda.device_count() in str(ei.value)
    with pytest.raises(B.BppError) as ei:
        B.VerifierPool(pk, N, CAP, window_bits=WB, devices=(0, torch.cuda.device_count()))
    assert ei.value.code == -2 and "shard 1 (device %d): " % torch.cuda.device_count() in str(ei.value)
    # two pools alive at once give the same verdicts
    other = B.VerifierPool(pk, N, CAP, window_bits=WB, devices=(0, 0))
    raw, cm = _u8(blobs), _u8(comms)
    assert pool.verify_serialized_mixed(raw, cm, ms).tolist() == other.verify_serialized_mixed(raw, cm, ms).tolist() == want
    other.close()
    upool.close()
    pool.close()
    # create / destroy ten times in a row
    for _ in range(10):
        q = B.VerifierPool(pk, N, CAP, window_bits=WB, devices=(0, 0))
        assert q.size == 2
        q.close()
