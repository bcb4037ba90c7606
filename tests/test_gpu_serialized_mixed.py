"""-m gpu: serialized proofs of mixed aggregation sizes (bpp_range_verify_batch_serialized_mixed_device) -- a block of
containers as bytes, proof i of shape (n, m_i), against one (n, m) verifier's tables.

Each status must be 2 (FormatError) where pyref's decoder rejects the container, else RangeProof::verify(proof_i,
PublicKey::new(n m_i), n, V_i): the definition with the PREFIX key of the proof's own shape.  Checked against the adversarial
corpus (tests/verdict_corpus.py) of every class encoded by pyref, against dedicated (n, m_i) verifiers' serialized path bit
for bit, under the transcript, for the locality of a FormatError, on the (64, 16) headline shape with a large device-proved
batch, for the usage errors, and through the host-pointer entry and the Python wrapper."""

import functools

import numpy as np
import pytest

import verdict_corpus as VC
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

CURVES = ("bls12_381", "secp256k1", "ed25519")
N, CAP, WB = 8, 4, 5
CLASSES = (1, 2, 4)


@functools.lru_cache(maxsize=None)
def _corpora(cname):
    return {m: VC.corpus(cname, N, m) for m in CLASSES}


def _interleave(cases_by_m, order):
    """(m, case index) pairs using every case of every class: the classes alternate in the pattern a b c a c b, so that
    each sits next to each other one; the batch starts with order[0] and ends with order[-1]"""
    a, b, c = order
    pattern = [a, b, c, a, c, b]
    used = {m: 0 for m in order}
    seq = []
    while any(used[m] < len(cases_by_m[m]) for m in order) or len(seq) < 6:
        m = pattern[len(seq) % 6]
        seq.append((m, used[m] % len(cases_by_m[m])))
        used[m] += 1
    seq.append((c, 0))
    return seq


def _u8(chunks):
    return np.frombuffer(b"".join(bytes(c) for c in chunks), dtype=np.uint8).copy()


def _run(torch, bv, blobs, comms, ms, transcript=False, uncompressed=False):
    """blobs / comms: per-proof byte strings -> status (count,) u32 through the device entry, caller order"""
    dev = torch.device("cuda:0")
    count = len(ms)
    d_p = torch.from_numpy(_u8(blobs)).to(dev)
    d_c = torch.from_numpy(_u8(comms)).to(dev)
    d_ok = torch.full((count,), 7, dtype=torch.int32, device=dev)
    wsb = bv.serialized_mixed_workspace_bytes(ms)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    bv.verify_serialized_mixed_device(d_p.data_ptr(), d_c.data_ptr(), ms, d_ok.data_ptr(), d_ws.data_ptr(), wsb,
                                      torch.cuda.current_stream().cuda_stream, transcript=transcript, uncompressed=uncompressed)
    torch.cuda.synchronize()
    return d_ok.cpu().numpy().astype(np.uint32)


def _run_single_shape(torch, bv, blobs, comms, transcript=False, uncompressed=False):
    """the single-shape serialized path (bpp_range_verify_batch_serialized_device) of verifier bv"""
    dev = torch.device("cuda:0")
    count = len(blobs)
    d_p = torch.from_numpy(_u8(blobs)).to(dev)
    d_c = torch.from_numpy(_u8(comms)).to(dev)
    d_ok = torch.full((count,), 7, dtype=torch.int32, device=dev)
    wsb = bv.serialized_workspace_bytes(count)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    bv.verify_serialized_device(d_p.data_ptr(), d_c.data_ptr(), count, d_ok.data_ptr(), d_ws.data_ptr(), wsb,
                                torch.cuda.current_stream().cuda_stream, transcript=transcript, uncompressed=uncompressed)
    torch.cuda.synchronize()
    return d_ok.cpu().numpy().astype(np.uint32)


def _setup(cname, transcript=False):
    import bulletproofsplus_amd as B
    cps = {m: VC.corpus(cname, N, m, transcript=True) for m in CLASSES} if transcript else _corpora(cname)
    cap = cps[CAP]
    a = B.Arith(cname)
    bv = B.BatchVerifier(B.PublicKey.from_points(a, cap.gh, cap.G, cap.H), N, CAP, window_bits=WB)
    return B, a, bv, cps


def _dedicated(B, a, cp, m):
    return B.BatchVerifier(B.PublicKey.from_points(a, cp.gh, cp.G, cp.H), N, m, window_bits=WB)


@pytest.mark.parametrize("cname", CURVES)
def test_serialized_mixed_matches_the_definition(cname):
    torch = need_gpu()
    B, a, bv, cps = _setup(cname)
    cases = {m: [c for c in cps[m].cases if c.status is not None] for m in CLASSES}
    # the share of cases without a container encoding is a condition of this test, not a result
    for m in CLASSES:
        left_out = len(cps[m].cases) - len(cases[m])
        print(cname, m, "cases", len(cases[m]), "left out", left_out, "statuses", sorted(c.status for c in cases[m]))
        assert len(cases[m]) >= 24 and left_out <= 5, (cname, m, len(cases[m]), left_out)
        seen = {c.status for c in cases[m]}
        assert {0, 1} <= seen and (2 in seen or cname == "secp256k1"), (cname, m, seen)
    for version in ((1, 2) if cname != "ed25519" else (1,)):
        enc = {m: [VC.encode_case(cps[m], c, version) for c in cases[m]] for m in CLASSES}
        for order in ((1, 2, 4), (2, 4, 1), (4, 1, 2)):
            seq = _interleave(cases, order)
            ms = [m for m, _ in seq]
            ok = _run(torch, bv, [enc[m][i][0] for m, i in seq], [enc[m][i][1] for m, i in seq], ms, uncompressed=version == 2)
            want = [cases[m][i].status for m, i in seq]
            bad = [(j, seq[j][0], cases[seq[j][0]][seq[j][1]].name, int(ok[j]), want[j]) for j in range(len(seq)) if ok[j] != want[j]]
            assert not bad, (version, order, bad)
    bv.close()


@pytest.mark.parametrize("cname", CURVES)
def test_serialized_mixed_equals_dedicated_verifiers(cname):
    torch = need_gpu()
    B, a, bv, cps = _setup(cname)
    cases = {m: [c for c in cps[m].cases if c.status is not None] for m in CLASSES}
    for version in ((1, 2) if cname != "ed25519" else (1,)):
        unc = version == 2
        enc = {m: [VC.encode_case(cps[m], c, version) for c in cases[m]] for m in CLASSES}
        seq = _interleave(cases, (2, 1, 4))
        ms = [m for m, _ in seq]
        blobs, comms = [enc[m][i][0] for m, i in seq], [enc[m][i][1] for m, i in seq]
        ok = _run(torch, bv, blobs, comms, ms, uncompressed=unc)
        for m in CLASSES:
            pos = [j for j, (mm, _) in enumerate(seq) if mm == m]
            ded = _dedicated(B, a, cps[m], m)
            dok = _run_single_shape(torch, ded, [blobs[j] for j in pos], [comms[j] for j in pos], uncompressed=unc)
            assert ok[pos].tolist() == dok.tolist(), (version, m)
            ded.close()
        # a batch of one class only; for the capacity class it is the verifier's own serialized path
        for m in CLASSES:
            idx = [i % len(cases[m]) for i in range(0, 3 * len(cases[m]), 3)][:9]
            b1, c1 = [enc[m][i][0] for i in idx], [enc[m][i][1] for i in idx]
            ok1 = _run(torch, bv, b1, c1, [m] * len(idx), uncompressed=unc)
            assert ok1.tolist() == [cases[m][i].status for i in idx], (version, m)
            if m == CAP:
                assert ok1.tolist() == _run_single_shape(torch, bv, b1, c1, uncompressed=unc).tolist()
    bv.close()


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_serialized_mixed_transcript(cname):
    torch = need_gpu()
    B, a, bv, cps = _setup(cname, transcript=True)
    cases = {m: list(cps[m].cases) for m in CLASSES}
    status = {m: [cps[m].container_status(c) for c in cases[m]] for m in CLASSES}
    by_name = {"valid_1": 0, "valid_2": 0, "flip_r": 1, "flip_s": 1, "flip_d": 1, "nc_r_plus_r": 2}
    for m in CLASSES:   # none may be left out
        names = [c.name for c in cases[m]]
        assert set(names) == set(by_name) - ({"nc_r_plus_r"} if cname == "secp256k1" else set()), names
        assert status[m] == [by_name[nm] for nm in names], (m, list(zip(names, status[m])))
    enc = {m: [VC.encode_case(cps[m], c) for c in cases[m]] for m in CLASSES}
    for order in ((4, 1, 2), (1, 2, 4)):
        seq = _interleave(cases, order)
        ms = [m for m, _ in seq]
        blobs, comms = [enc[m][i][0] for m, i in seq], [enc[m][i][1] for m, i in seq]
        ok = _run(torch, bv, blobs, comms, ms, transcript=True)
        assert ok.tolist() == [status[m][i] for m, i in seq], order
        for m in CLASSES:
            pos = [j for j, (mm, _) in enumerate(seq) if mm == m]
            ded = _dedicated(B, a, cps[m], m)
            dok = _run_single_shape(torch, ded, [blobs[j] for j in pos], [comms[j] for j in pos], transcript=True)
            assert ok[pos].tolist() == dok.tolist(), m
            ded.close()
    # the transcript binds the proof: with the literal challenges the same valid proofs fail
    seq = [(m, 0) for m in CLASSES]
    ok = _run(torch, bv, [enc[m][0][0] for m, _ in seq], [enc[m][0][1] for m, _ in seq], list(CLASSES))
    assert ok.tolist() == [1, 1, 1]
    bv.close()


@pytest.mark.parametrize("cname", CURVES)
def test_format_error_is_local(cname):
    """one corrupted container at a time in an all-valid interleaved batch: exactly that proof reads 2"""
    torch = need_gpu()
    B, a, bv, cps = _setup(cname)
    cases = {m: [c for c in cps[m].cases if c.status == 0][:5] for m in CLASSES}
    assert all(len(cases[m]) >= 4 for m in CLASSES)
    enc = {m: [VC.encode_case(cps[m], c) for c in cases[m]] for m in CLASSES}
    seq = _interleave(cases, (2, 4, 1))
    ms = [m for m, _ in seq]
    blobs, comms = [enc[m][i][0] for m, i in seq], [enc[m][i][1] for m, i in seq]
    assert _run(torch, bv, blobs, comms, ms).tolist() == [0] * len(seq)
    # first and last proof of the batch, first and last proof of every class region (caller order within a class)
    targets = {0, len(seq) - 1}
    for m in CLASSES:
        pos = [j for j, mm in enumerate(ms) if mm == m]
        targets |= {pos[0], pos[-1]}
    r_le = cps[CAP].r.to_bytes(32, "little")

    def corruptions(blob, m):
        other = next(x for x in CLASSES if x != m)
        for what, at, val in (("m", 7, other), ("k", 8, blob[8] + 1), ("reserved", 10, 1),
                              ("flags", 12, {"bls12_381": blob[12] & 0x7f, "secp256k1": 4, "ed25519": blob[12] | 1}[cname])):
            b = bytearray(blob)
            assert b[at] != val
            b[at] = val
            yield what, bytes(b)
        yield "scalar = r", blob[:-32] + r_le
        yield "scalar r' = r", blob[:-96] + r_le + blob[-64:]

    for j in sorted(targets):
        for what, bad in corruptions(blobs[j], ms[j]):
            ok = _run(torch, bv, blobs[:j] + [bad] + blobs[j + 1:], comms, ms)
            assert ok.tolist() == [2 if t == j else 0 for t in range(len(seq))], (j, ms[j], what, ok.tolist())
        # ... and a commitment that does not parse
        cbad = bytearray(comms[j])
        cbad[0] = {"bls12_381": cbad[0] & 0x7f, "secp256k1": 4, "ed25519": cbad[0] | 1}[cname]
        ok = _run(torch, bv, blobs, comms[:j] + [bytes(cbad)] + comms[j + 1:], ms)
        assert ok.tolist() == [2 if t == j else 0 for t in range(len(seq))], (j, ms[j], "commitment", ok.tolist())
    bv.close()


def test_serialized_mixed_big_shape():
    """capacity (64, 16) at window 8 on BLS12-381: 4 096 device-proved (64,1) proofs and 256 (64,16) ones encoded by the
    product per class, shuffled, a few tampered and a few with a corrupted encoding, against the dedicated verifiers'
    serialized path; then class lane counts that are not multiples of the wave size, and a batch of one"""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cname, n, M = "bls12_381", 64, 16
    big = VC.corpus(cname, n, M)
    a = B.Arith(cname)
    bv = B.BatchVerifier(B.PublicKey.from_points(a, big.gh, big.G, big.H), n, M, window_bits=8)
    e1 = B.BatchVerifier(B.PublicKey.from_points(a, big.gh, big.G[:n], big.H[:n]), n, 1, window_bits=8)
    rng = np.random.default_rng(7)
    p1, s1, V1 = e1.prove_batch(rng.integers(0, 1 << 31, size=(4096, 1), dtype=np.uint64).tolist(),
                                [[int(x)] for x in rng.integers(1, 1 << 62, size=4096)])
    p16, s16, V16 = bv.prove_batch(rng.integers(0, 1 << 31, size=(256, M), dtype=np.uint64).tolist(),
                                   [[int(x) for x in row] for row in rng.integers(1, 1 << 62, size=(256, M))])
    for t in (3, 1000, 4095):
        s1[t, 1, 0] ^= 1
    for t in (0, 200):
        s16[t, 1, 0] ^= 1
    b1 = B.encode_proofs(a, n, 1, p1, s1)
    b16 = B.encode_proofs(a, n, M, p16, s16)
    c1 = B.compress_points(a, V1.reshape(-1, a.PW)).reshape(4096, -1)
    c16 = B.compress_points(a, V16.reshape(-1, a.PW)).reshape(256, -1)
    assert b1.shape[1] == B.proof_bytes(a, n, 1) and b16.shape[1] == B.proof_bytes(a, n, M)
    b1[7, 12] &= 0x7f                # a point's flag bits
    b1[2048, 8] += 1                 # k
    b1[4000, -32:] = np.frombuffer(big.r.to_bytes(32, "little"), np.uint8)
    b16[5, 7] = 8                    # another m
    b16[255, 12 + 48 * 9] &= 0x7f
    c16[100, 48 * 15] &= 0x7f        # the last commitment
    d1 = _run_single_shape(torch, e1, list(b1), list(c1))
    d16 = _run_single_shape(torch, bv, list(b16), list(c16))
    assert sorted(np.flatnonzero(d1 == 1).tolist()) == [3, 1000, 4095] and sorted(np.flatnonzero(d1 == 2).tolist()) == [7, 2048, 4000]
    assert sorted(np.flatnonzero(d16 == 1).tolist()) == [0, 200] and sorted(np.flatnonzero(d16 == 2).tolist()) == [5, 100, 255]
    order = rng.permutation(4096 + 256)
    blobs = [b1[i] if i < 4096 else b16[i - 4096] for i in order]
    comms = [c1[i] if i < 4096 else c16[i - 4096] for i in order]
    ms = [1 if i < 4096 else M for i in order]
    ok = _run(torch, bv, blobs, comms, ms)
    assert np.array_equal(ok, np.array([d1[i] if i < 4096 else d16[i - 4096] for i in order]))
    assert np.array_equal(bv.verify_serialized_mixed(_u8(blobs), _u8(comms), ms), ok)     # the host-pointer entry
    # lane counts that are not multiples of 64: 5 x 16 and 3 x 39 record points; and single proofs
    pick = [(1, 3), (16, 0), (1, 4), (1, 7), (16, 5), (1, 8), (16, 9), (1, 9)]
    blobs = [b1[i] if m == 1 else b16[i] for m, i in pick]
    comms = [c1[i] if m == 1 else c16[i] for m, i in pick]
    assert _run(torch, bv, blobs, comms, [m for m, _ in pick]).tolist() == [d1[i] if m == 1 else d16[i] for m, i in pick]
    for m, i in ((1, 5), (1, 7), (16, 1), (16, 0), (16, 5)):
        assert _run(torch, bv, [b1[i] if m == 1 else b16[i]], [c1[i] if m == 1 else c16[i]], [m]).tolist() == \
            [d1[i] if m == 1 else d16[i]], (m, i)
    e1.close()
    bv.close()


def test_serialized_mixed_arguments():
    torch = need_gpu()
    from bulletproofsplus_amd import _lib
    B, a, bv, cps = _setup("secp256k1")
    good = [cps[m].by_name("valid_1") for m in CLASSES]
    enc = [VC.encode_case(cps[m], c) for m, c in zip(CLASSES, good)]
    dev = torch.device("cuda:0")
    d_p = torch.from_numpy(_u8([e[0] for e in enc])).to(dev)
    d_c = torch.from_numpy(_u8([e[1] for e in enc])).to(dev)
    d_ok = torch.full((3,), 7, dtype=torch.int32, device=dev)
    wsb = bv.serialized_mixed_workspace_bytes(list(CLASSES))
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    args = (d_ok.data_ptr(), d_ws.data_ptr(), wsb, st)
    for bad_ms, where in (([1, 3, 4], 1), ([1, 2, 2 * CAP], 2), ([0, 2, 4], 0)):
        assert bv.serialized_mixed_workspace_bytes(bad_ms) == 0
        with pytest.raises(B.BppError) as ei:
            bv.verify_serialized_mixed_device(d_p.data_ptr(), d_c.data_ptr(), bad_ms, *args)
        assert ei.value.code == -1 and ("m_of[%d]" % where) in str(ei.value), str(ei.value)
        with pytest.raises(B.BppError):
            bv.verify_serialized_mixed(d_p.cpu().numpy(), d_c.cpu().numpy(), bad_ms)
    with pytest.raises(B.BppError) as ei:
        bv.verify_serialized_mixed_device(d_p.data_ptr(), d_c.data_ptr(), list(CLASSES), d_ok.data_ptr(), d_ws.data_ptr(),
                                          wsb - 1, st)
    assert ei.value.code == -1 and "workspace" in str(ei.value)
    m3 = bv._ms(CLASSES)
    with pytest.raises(B.BppError) as ei:    # ristretto255 aside, secp256k1 takes version 2; an unknown flag is a usage error
        _lib.check(_lib.lib().bpp_range_verify_batch_serialized_mixed_device(
            bv.handle, d_p.data_ptr(), d_c.data_ptr(), m3.ctypes.data, 3, 4, d_ok.data_ptr(), d_ws.data_ptr(), wsb,
            None), "flags")
    assert ei.value.code == -1
    for null_at in (1, 2, 3, 6, 7):
        argv = [bv.handle, d_p.data_ptr(), d_c.data_ptr(), m3.ctypes.data, 3, 0, d_ok.data_ptr(), d_ws.data_ptr(),
                wsb, None]
        argv[null_at] = None
        assert _lib.lib().bpp_range_verify_batch_serialized_mixed_device(*argv) == -1, null_at
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [7, 7, 7]
    bv.verify_serialized_mixed_device(d_p.data_ptr(), d_c.data_ptr(), [], *args)
    assert _lib.lib().bpp_range_verify_batch_serialized_mixed(bv.handle, None, None, None, 0, 0, None) == 0
    assert bv.verify_serialized_mixed(b"", b"").tolist() == []
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [7, 7, 7]
    bv.verify_serialized_mixed_device(d_p.data_ptr(), d_c.data_ptr(), list(CLASSES), *args)
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [c.status for c in good] == [0, 0, 0]
    # version 2 has no ristretto255 form
    B2, a2, bv2, cps2 = _setup("ed25519")
    with pytest.raises(B.BppError):
        bv2.verify_serialized_mixed_device(d_p.data_ptr(), d_c.data_ptr(), list(CLASSES), *args, uncompressed=True)
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [0, 0, 0]
    bv2.close()
    bv.close()


@pytest.mark.parametrize("cname", ("bls12_381", "ed25519"))
def test_serialized_mixed_host_entry_and_wrapper(cname):
    torch = need_gpu()
    B, a, bv, cps = _setup(cname)
    cases = {m: [c for c in cps[m].cases if c.status is not None] for m in CLASSES}
    enc = {m: [VC.encode_case(cps[m], c) for c in cases[m]] for m in CLASSES}
    seq = _interleave(cases, (1, 4, 2))
    ms = [m for m, _ in seq]
    blobs, comms = [enc[m][i][0] for m, i in seq], [enc[m][i][1] for m, i in seq]
    ok = _run(torch, bv, blobs, comms, ms)
    assert ok.tolist() == [cases[m][i].status for m, i in seq]
    raw, cm = b"".join(blobs), b"".join(comms)
    assert bv.verify_serialized_mixed(raw, cm, ms).tolist() == ok.tolist()
    assert bv.verify_serialized_mixed(_u8(blobs), _u8(comms), np.array(ms)).tolist() == ok.tolist()
    # without ms the wrapper frames the stream itself: every header of this corpus names its own shape
    assert B.proofs_scan(a, N, raw).tolist() == ms
    assert bv.verify_serialized_mixed(raw, cm).tolist() == ok.tolist()
    with pytest.raises(B.BppError) as ei:
        bv.verify_serialized_mixed(raw[:-1], cm)
    assert "container %d " % (len(ms) - 1) in str(ei.value)
    with pytest.raises(RuntimeError):
        bv.verify_serialized_mixed(raw, cm, ms[:-1] + [ms[-1] * 2 if ms[-1] < CAP else 1])
    with pytest.raises(RuntimeError):
        bv.verify_serialized_mixed(raw, cm[:-1], ms)
    bv.close()
