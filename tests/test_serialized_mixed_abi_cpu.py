"""CPU: the serialized mixed-batch entry points (bpp_proofs_scan, bpp_range_verify_batch_serialized_mixed and friends) are
declared, exported and bound; their usage errors are return codes, not crashes; and the host-side framing of a bare byte
stream (bpp_proofs_scan, csrc/container_scan.hpp) recovers m_i per container from streams made by pyref's encoder -- in the
library, and in a host build that walks prefixes and mutations of those streams under the sanitizers (BPP_HOST_SANITIZE=1).
No GPU needed: nothing here reaches a device."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import verdict_corpus as VC
from test_host_arith_cpu import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bpp_proofs_scan", "bpp_verifier_serialized_mixed_workspace_bytes",
           "bpp_range_verify_batch_serialized_mixed_device", "bpp_range_verify_batch_serialized_mixed")
CURVES = ("bls12_381", "secp256k1", "ed25519")
N = 8
# container bytes at n = 8, version 1, m' = 1 / 2 / 4 (pyref's encoder)
LENGTHS = {"bls12_381": (540, 636, 732), "secp256k1": (405, 471, 537), "ed25519": (396, 460, 524)}
PATTERN = (1, 2, 4, 4, 1, 2, 2, 4, 1, 1)


def _lib():
    from bulletproofsplus_amd import _lib as M
    return M.lib()


def _stream(cname, version=1, pattern=PATTERN):
    """-> (bytes, [m per container]): valid containers of classes 1, 2, 4 interleaved, pyref-encoded"""
    blobs = []
    for j, m in enumerate(pattern):
        cp = VC.corpus(cname, N, m)
        blobs.append(VC.encode_case(cp, cp.by_name("valid_1" if j % 2 else "valid_2"), version)[0])
    return b"".join(blobs), list(pattern), [len(b) for b in blobs]


def _scan(cid, n, version, data, max_count):
    L = _lib()
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    m_of = np.full(max(max_count, 1) + 2, 0xdeadbeef, dtype=np.uint32)   # two guard words behind max_count
    cnt = ctypes.c_size_t(12345)
    rc = L.bpp_proofs_scan(cid, n, version, raw.ctypes.data_as(ctypes.c_void_p) if len(raw) else None, len(raw),
                           m_of.ctypes.data_as(ctypes.c_void_p), max_count, ctypes.byref(cnt))
    assert m_of[max(max_count, 1):].tolist() == [0xdeadbeef] * 2
    assert cnt.value <= max_count
    return rc, m_of[:cnt.value].tolist(), L.bpp_last_error().decode()


def test_symbols_are_declared_exported_and_bound():
    from bulletproofsplus_amd import _lib as M
    L = M.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpp_amd.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in M.EXPORTS, s
        assert hasattr(L, s), s
        assert "pub fn %s(" % s in ffi, s


def test_null_arguments_are_errors():
    L = _lib()
    ms = np.array([1, 2, 4], dtype=np.uint32)
    pm = ms.ctypes.data_as(ctypes.c_void_p)
    buf = np.zeros(64, dtype=np.uint64)
    pb = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.bpp_verifier_serialized_mixed_workspace_bytes(None, pm, 3) == 0
    assert L.bpp_verifier_serialized_mixed_workspace_bytes(None, None, 0) == 0
    assert L.bpp_range_verify_batch_serialized_mixed_device(None, pb, pb, pm, 3, 0, pb, pb, 1 << 20, None) < 0
    assert "null" in L.bpp_last_error().decode()
    assert L.bpp_range_verify_batch_serialized_mixed_device(None, None, None, None, 3, 0, None, None, 0, None) < 0
    assert L.bpp_range_verify_batch_serialized_mixed_device(None, None, None, None, 0, 0, None, None, 0, None) < 0
    assert L.bpp_range_verify_batch_serialized_mixed(None, pb, pb, pm, 3, 0, pb) < 0
    assert L.bpp_range_verify_batch_serialized_mixed(None, None, None, None, 3, 1, None) < 0
    assert "null" in L.bpp_last_error().decode()
    cnt = ctypes.c_size_t(0)
    assert L.bpp_proofs_scan(0, N, 1, None, 10, pm, 3, ctypes.byref(cnt)) < 0
    assert "null" in L.bpp_last_error().decode()
    assert L.bpp_proofs_scan(0, N, 1, pb, 10, None, 3, ctypes.byref(cnt)) < 0
    assert L.bpp_proofs_scan(0, N, 1, pb, 10, pm, 3, None) < 0
    # curve, version, n the walk does not take
    for cid, n, version in ((9, N, 1), (0, N, 3), (2, N, 2), (0, 0, 1), (0, 6, 1), (0, 256, 1)):
        assert L.bpp_proofs_scan(cid, n, version, pb, 10, pm, 3, ctypes.byref(cnt)) < 0, (cid, n, version)


@pytest.mark.parametrize("cname", CURVES)
def test_scan_frames_a_mixed_stream(cname):
    cid = VC.CID[cname]
    data, ms, lens = _stream(cname)
    for m, ln in zip(ms, lens):
        assert ln == LENGTHS[cname][(1, 2, 4).index(m)], (cname, m, ln)
        assert ln == _lib().bpp_proof_bytes_version(cid, N, m, 1)
    assert _scan(cid, N, 1, data, len(ms))[:2] == (0, ms)
    assert _scan(cid, N, 1, data, len(ms) + 5)[:2] == (0, ms)
    assert _scan(cid, N, 1, b"", 4)[:2] == (0, [])
    assert _scan(cid, N, 1, b"", 0)[:2] == (0, [])
    starts = np.concatenate([[0], np.cumsum(lens)]).tolist()

    def rejected(blob, max_count, index, word):
        rc, got, err = _scan(cid, N, 1, blob, max_count)
        assert rc < 0 and got == ms[:index], (rc, got, err)
        assert ("container %d " % index) in err and ("byte %d" % starts[index]) in err and word in err, err

    rejected(data[:-1], len(ms), len(ms) - 1, "truncated")                       # a truncated tail
    rejected(data[:starts[4] + 7], len(ms), 4, "truncated")                      # ... inside a header
    rejected(data + b"BPP+", len(ms) + 1, len(ms), "truncated")
    bad = bytearray(data)
    bad[starts[2] + 1] ^= 0x20
    rejected(bad, len(ms), 2, "magic")                                           # a flipped magic byte, third container
    bad = bytearray(data)
    bad[starts[3] + 7] = 3
    rejected(bad, len(ms), 3, "m ")                                              # m = 3
    bad = bytearray(data)
    bad[starts[5] + 8] += 1
    rejected(bad, len(ms), 5, "k ")                                              # k off by one
    bad = bytearray(data)
    bad[starts[1] + 7] = 4                                                       # another class's m under this k
    rejected(bad, len(ms), 1, "k ")
    bad = bytearray(data)
    bad[starts[6] + 5] = (cid + 1) % 3
    rejected(bad, len(ms), 6, "curve")
    bad = bytearray(data)
    bad[starts[0] + 4] = 2
    rejected(bad, len(ms), 0, "version")
    bad = bytearray(data)
    bad[starts[9] + 6] = 4
    rejected(bad, len(ms), 9, "n ")
    rejected(data, len(ms) - 1, len(ms) - 1, "max_count")                        # max_count too small
    rejected(data, 3, 3, "max_count")
    # what the walk does not need, it does not judge: reserved bytes, encodings and scalars are the decoder's business
    ok = bytearray(data)
    ok[starts[2] + 10] = 1
    ok[starts[2] + 12] ^= 0xff
    ok[-1] = 0xff
    assert _scan(cid, N, 1, ok, len(ms))[:2] == (0, ms)


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_scan_version_2(cname):
    cid = VC.CID[cname]
    data, ms, lens = _stream(cname, 2)
    for m, ln in zip(ms, lens):
        assert ln == _lib().bpp_proof_bytes_version(cid, N, m, 2)
    assert _scan(cid, N, 2, data, len(ms))[:2] == (0, ms)
    rc, got, err = _scan(cid, N, 1, data, len(ms))
    assert rc < 0 and got == [] and "container 0 " in err and "version" in err
    rc, got, err = _scan(cid, N, 2, data[:-40], len(ms))
    assert rc < 0 and got == ms[:-1] and ("container %d " % (len(ms) - 1)) in err


def test_python_wrapper_scans():
    import bulletproofsplus_amd as B
    data, ms, _ = _stream("secp256k1")
    a = "secp256k1"                       # an Arith or a curve name: the scan needs no context and no device
    assert B.proofs_scan(a, N, data).tolist() == ms
    assert B.proofs_scan(a, N, np.frombuffer(data, dtype=np.uint8)).tolist() == ms
    assert B.proofs_scan(a, N, b"").tolist() == []
    with pytest.raises(B.BppError) as ei:
        B.proofs_scan(a, N, data[:-3])
    assert ei.value.code < 0 and "container %d " % (len(ms) - 1) in str(ei.value)


@pytest.mark.parametrize("cname,version", [(c, 1) for c in CURVES] + [("bls12_381", 2), ("secp256k1", 2)])
def test_scan_host_build_walks_prefixes_and_mutations(cname, version, tmp_path):
    """csrc/container_scan.hpp under g++ (ASan + UBSan with BPP_HOST_SANITIZE=1): exact-size buffers, so a read past
    proofs_bytes or more than max_count outputs is a reported overflow"""
    exe = _build("container_scan_host_test", tmp_path)
    data, ms, _ = _stream(cname, version)
    path = tmp_path / ("stream_%s_%d.bin" % (cname, version))
    path.write_bytes(data)
    out = subprocess.run([exe, str(VC.CID[cname]), str(N), str(version), str(path), ",".join(map(str, ms))],
                         capture_output=True, text=True)
    assert out.returncode == 0 and "ok container_scan" in out.stdout, out.stdout + out.stderr
