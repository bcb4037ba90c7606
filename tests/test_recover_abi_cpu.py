"""CPU: the mask-recovery and scan entry points (bpp_range_recover_masks_mixed*, bpp_range_scan_serialized_mixed* and their
workspace functions) are declared, exported, bound and present in the Rust FFI; they run under the entry shim; their usage
errors are return codes that leave the caller's buffers alone.  No GPU needed: every case here is answered by an argument
check before the engine handle is read, so a dummy non-null handle stands in for one.  The two cases that need the engine's
shape -- an m_i above its m, a workspace smaller than the layout -- are in tests/test_gpu_recover.py."""

import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bpp_recover_mixed_workspace_bytes", "bpp_range_recover_masks_mixed_device", "bpp_range_recover_masks_mixed",
           "bpp_scan_serialized_mixed_workspace_bytes", "bpp_range_scan_serialized_mixed_device",
           "bpp_range_scan_serialized_mixed")
TRANSCRIPT, UNCOMPRESSED, AMOUNT64 = 1, 2, 0x100
KEY = bytes(range(32))


def _lib():
    from bulletproofsplus_amd import _lib as M
    return M.lib()


def _bufs():
    buf = np.full(64, 0x77, dtype=np.uint64)
    return buf, buf.ctypes.data_as(ctypes.c_void_p)


def _err():
    return _lib().bpp_last_error().decode()


def test_symbols_are_declared_exported_and_bound():
    from bulletproofsplus_amd import _lib as M
    from bulletproofsplus_amd import api
    L = M.lib()
    raw = open(os.path.join(ROOT, "include", "bpp_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in M.EXPORTS, s
        assert hasattr(L, s), s
        assert "pub fn %s(" % s in ffi, s
    m = re.search(r"^#define\s+BPP_SCAN_UNCONFIRMED\s+(\S+)\s*$", hdr, flags=re.M)
    assert m and int(m.group(1), 0) == 3 == api.SCAN_UNCONFIRMED
    assert re.search(r"pub const BPP_SCAN_UNCONFIRMED: \w+ = 3;", ffi)
    # the header says what a scan is not, what the key is, and cites the quantities inverted
    block = raw[raw.index("mask recovery (\"rewind\") and scanning"):raw.index("size_t bpp_recover_mixed_workspace_bytes(")]
    for text in ("A SCAN IS NOT A VERIFICATION", "Scan what has been verified", "VIEW KEY", "a key never meets an index twice",
                 "src/range/mod.rs:159-172", "src/weighted_inner_product_proof.rs:94-95,175-227"):
        assert text in block, text


def test_entries_run_under_the_guard():
    import test_abi_guard_cpu as G
    entries = G._entry_points(open(os.path.join(ROOT, "bulletproofsplus_amd", "csrc", "capi.hip")).read())
    for s in SYMBOLS:
        assert s in entries and any(shim in entries[s] for shim in G.SHIMS), s
        if "workspace_bytes" not in s:
            assert '{count, "count"}' in entries[s], (s, "count is not bounded by the shim")


def test_wrappers_exist():
    import bulletproofsplus_amd as B
    for name in ("recover_masks", "recover_masks_device", "scan_serialized_mixed", "scan_serialized_mixed_device",
                 "recover_workspace_bytes"):
        assert callable(getattr(B.BatchVerifier, name)), name


def _recover_device(L, v, sc, pm, count, ch, key, idx, bl, out, ws, wsb):
    return L.bpp_range_recover_masks_mixed_device(v, sc, pm, count, ch, key, 5, idx, bl, out, ws, wsb, None)


def _recover_host(L, v, sc, pm, count, ch, key, idx, bl, out):
    return L.bpp_range_recover_masks_mixed(v, sc, pm, count, ch, key, 5, idx, bl, out)


def _scan_device(L, v, pr, cm, pm, count, flags, key, idx, bl, am, out, st, ws, wsb):
    return L.bpp_range_scan_serialized_mixed_device(v, pr, cm, pm, count, flags, key, 5, idx, bl, am, out, st, ws, wsb, None)


def _scan_host(L, v, pr, cm, pm, count, flags, key, idx, bl, am, out, st):
    return L.bpp_range_scan_serialized_mixed(v, pr, cm, pm, count, flags, key, 5, idx, bl, am, out, st)


def test_recover_usage_errors_leave_the_buffers_alone():
    L = _lib()
    buf, pb = _bufs()
    eng = pb   # never read
    ms = np.array([1, 2, 4], dtype=np.uint32)
    pm = ms.ctypes.data_as(ctypes.c_void_p)
    # a NULL engine, with work and without
    for count in (3, 0):
        assert _recover_device(L, None, pb, pm, count, pb, KEY, None, None, pb, pb, 1 << 20) < 0 and "null" in _err()
        assert _recover_host(L, None, pb, pm, count, pb, KEY, None, None, pb) < 0 and "null" in _err()
    # a NULL required pointer: scalars, m_of, the output, the workspace
    for args in ((None, pm, pb, pb), (pb, None, pb, pb), (pb, pm, None, pb), (pb, pm, pb, None)):
        assert _recover_device(L, eng, args[0], args[1], 3, None, KEY, None, None, args[2], args[3], 1 << 20) < 0
        assert "null" in _err()
    for args in ((None, pm, pb), (pb, None, pb), (pb, pm, None)):
        assert _recover_host(L, eng, args[0], args[1], 3, None, KEY, None, None, args[2]) < 0 and "null" in _err()
    # both blinding sources; an index without a key
    assert _recover_device(L, eng, pb, pm, 3, None, KEY, None, pb, pb, pb, 1 << 20) < 0 and "both" in _err()
    assert _recover_host(L, eng, pb, pm, 3, None, KEY, None, pb, pb) < 0 and "both" in _err()
    assert _recover_device(L, eng, pb, pm, 3, None, None, pb, None, pb, pb, 1 << 20) < 0 and "d_index" in _err()
    assert _recover_device(L, eng, pb, pm, 3, None, None, pb, pb, pb, pb, 1 << 20) < 0 and "d_index" in _err()
    assert _recover_host(L, eng, pb, pm, 3, None, None, pb, None, pb) < 0 and "d_index" in _err()
    # an m_i no engine takes: the text names i
    for bad, at in (([1, 3, 2], 1), ([0, 1, 1], 0), ([2, 4, 12], 2)):
        b = np.array(bad, dtype=np.uint32)
        pbad = b.ctypes.data_as(ctypes.c_void_p)
        assert _recover_device(L, eng, pb, pbad, 3, None, KEY, None, None, pb, pb, 1 << 20) < 0 and "m_of[%d]" % at in _err()
        assert _recover_host(L, eng, pb, pbad, 3, None, KEY, None, None, pb) < 0 and "m_of[%d]" % at in _err()
        assert L.bpp_recover_mixed_workspace_bytes(eng, pbad, 3) == 0
    # a workspace of no bytes
    assert _recover_device(L, eng, pb, pm, 3, None, KEY, None, None, pb, pb, 0) < 0 and "workspace too small" in _err()
    # count = 0 is BPP_OK, whatever else is NULL
    assert _recover_device(L, eng, None, None, 0, None, None, None, None, None, None, 0) == 0
    assert _recover_host(L, eng, None, None, 0, None, None, None, None, None) == 0
    assert L.bpp_recover_mixed_workspace_bytes(None, pm, 3) == 0
    assert L.bpp_recover_mixed_workspace_bytes(eng, None, 3) == 0
    assert buf.tolist() == [0x77] * 64   # nothing was written


def test_scan_usage_errors_leave_the_buffers_alone():
    L = _lib()
    buf, pb = _bufs()
    eng = pb   # never read
    ms = np.array([1, 2, 4], dtype=np.uint32)
    pm = ms.ctypes.data_as(ctypes.c_void_p)
    T = TRANSCRIPT
    for count in (3, 0):
        assert _scan_device(L, None, pb, pb, pm, count, T, KEY, None, None, pb, pb, pb, pb, 1 << 20) < 0 and "null" in _err()
        assert _scan_host(L, None, pb, pb, pm, count, T, KEY, None, None, pb, pb, pb) < 0 and "null" in _err()
    # a NULL required pointer: proofs, commitments, m_of, masks, status, workspace (the amounts may be NULL)
    for i in range(6):
        a = [pb, pb, pm, pb, pb, pb]
        a[i] = None
        assert _scan_device(L, eng, a[0], a[1], a[2], 3, T, KEY, None, None, None, a[3], a[4], a[5], 1 << 20) < 0 and "null" in _err()
    for i in range(5):
        a = [pb, pb, pm, pb, pb]
        a[i] = None
        assert _scan_host(L, eng, a[0], a[1], a[2], 3, T, KEY, None, None, None, a[3], a[4]) < 0 and "null" in _err()
    # unknown flags, also with count = 0; the three known ones pass the flag check
    for fl in (4, 8, 0x200, AMOUNT64 | 4, -1):
        for count in (3, 0):
            assert _scan_device(L, eng, pb, pb, pm, count, fl, None, None, None, None, pb, pb, pb, 1 << 20) < 0
            assert "unknown flag" in _err(), fl
            assert _scan_host(L, eng, pb, pb, pm, count, fl, None, None, None, None, pb, pb) < 0 and "unknown flag" in _err()
    for fl in (T, T | UNCOMPRESSED, T | AMOUNT64, T | UNCOMPRESSED | AMOUNT64, 0, AMOUNT64):
        assert _scan_device(L, eng, None, None, pm, 3, fl, None, None, None, None, pb, pb, pb, 1 << 20) < 0
        assert "null" in _err() and "unknown flag" not in _err(), hex(fl)
    # both blinding sources; an index without a key; blinding without the transcript
    assert _scan_device(L, eng, pb, pb, pm, 3, T, KEY, None, pb, None, pb, pb, pb, 1 << 20) < 0 and "both" in _err()
    assert _scan_host(L, eng, pb, pb, pm, 3, T, KEY, None, pb, None, pb, pb) < 0 and "both" in _err()
    assert _scan_device(L, eng, pb, pb, pm, 3, T, None, pb, None, None, pb, pb, pb, 1 << 20) < 0 and "d_index" in _err()
    assert _scan_host(L, eng, pb, pb, pm, 3, T, None, pb, None, None, pb, pb) < 0 and "d_index" in _err()
    for fl in (0, UNCOMPRESSED, AMOUNT64):
        assert _scan_device(L, eng, pb, pb, pm, 3, fl, KEY, None, None, None, pb, pb, pb, 1 << 20) < 0
        assert "BPP_SER_TRANSCRIPT" in _err()
        assert _scan_device(L, eng, pb, pb, pm, 3, fl, None, None, pb, None, pb, pb, pb, 1 << 20) < 0
        assert "BPP_SER_TRANSCRIPT" in _err()
        assert _scan_host(L, eng, pb, pb, pm, 3, fl, KEY, None, None, None, pb, pb) < 0 and "BPP_SER_TRANSCRIPT" in _err()
    # an m_i no engine takes: the text names i
    for bad, at in (([1, 3, 2], 1), ([0, 1, 1], 0), ([2, 4, 12], 2)):
        b = np.array(bad, dtype=np.uint32)
        pbad = b.ctypes.data_as(ctypes.c_void_p)
        assert _scan_device(L, eng, pb, pb, pbad, 3, T, KEY, None, None, None, pb, pb, pb, 1 << 20) < 0 and "m_of[%d]" % at in _err()
        assert _scan_host(L, eng, pb, pb, pbad, 3, T, KEY, None, None, None, pb, pb) < 0 and "m_of[%d]" % at in _err()
        assert L.bpp_scan_serialized_mixed_workspace_bytes(eng, pbad, 3) == 0
    assert _scan_device(L, eng, pb, pb, pm, 3, T, KEY, None, None, None, pb, pb, pb, 0) < 0 and "workspace too small" in _err()
    # count = 0 is BPP_OK
    assert _scan_device(L, eng, None, None, None, 0, T, None, None, None, None, None, None, None, 0) == 0
    assert _scan_host(L, eng, None, None, None, 0, T | AMOUNT64, None, None, None, None, None, None) == 0
    assert L.bpp_scan_serialized_mixed_workspace_bytes(None, pm, 3) == 0
    assert L.bpp_scan_serialized_mixed_workspace_bytes(eng, None, 3) == 0
    assert buf.tolist() == [0x77] * 64   # nothing was written
