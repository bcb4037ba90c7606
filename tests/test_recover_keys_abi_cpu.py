"""CPU: the many-key scan entry points (bpp_scan_serialized_mixed_keys_workspace_bytes,
bpp_range_scan_serialized_mixed_keys_device, bpp_range_scan_serialized_mixed_keys) are declared, exported, bound and present
in the Rust FFI; they run under the entry shim; the Python, C++ and Rust wrappers exist; their usage errors are BPP_E_ARG
and leave the caller's buffers alone.  No GPU needed: every case here is answered by an argument check before the engine
handle is read, so a dummy non-null handle stands in for one.  The case that needs the engine's shape -- a workspace
smaller than the layout -- is in tests/test_gpu_recover_keys.py."""

import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bpp_scan_serialized_mixed_keys_workspace_bytes", "bpp_range_scan_serialized_mixed_keys_device",
           "bpp_range_scan_serialized_mixed_keys")
TRANSCRIPT, UNCOMPRESSED, AMOUNT64 = 1, 2, 0x100
E_ARG = -1
BOUND = 0x7fffffff // 64


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
    L = M.lib()
    raw = open(os.path.join(ROOT, "include", "bpp_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in M.EXPORTS, s
        assert hasattr(L, s), s
        assert "pub fn %s(" % s in ffi, s
    # the header repeats the view-key warning, names the layouts and the size of the output
    block = raw[raw.index("scanning a block under MANY keys"):raw.index("size_t bpp_scan_serialized_mixed_keys_workspace_bytes(")]
    for text in ("VIEW KEY", "A SCAN IS NOT A VERIFICATION", "KEY-MAJOR", "36 bytes of output per pair", "SHARED BY ALL KEYS",
                 "overwrites that buffer before freeing it", "BPP_SER_TRANSCRIPT (REQUIRED"):
        assert text in block, text


def test_entries_run_under_the_guard():
    import test_abi_guard_cpu as G
    entries = G._entry_points(open(os.path.join(ROOT, "bulletproofsplus_amd", "csrc", "capi.hip")).read())
    for s in SYMBOLS:
        assert s in entries and any(shim in entries[s] for shim in G.SHIMS), s
        if "workspace_bytes" not in s:
            assert '{count, "count"}' in entries[s], (s, "count is not bounded by the shim")
            assert "scan_args(SCAN_MANY_KEYS_" in entries[s] and "pairs_bounded(a.n_keys, a.count)" in G._receiver_check("scan_args"), \
                (s, "n_keys x count is not bounded before the engine is read")


def test_wrappers_exist():
    import bulletproofsplus_amd as B
    for name in ("scan_serialized_mixed_keys", "scan_serialized_mixed_keys_device", "scan_keys_workspace_bytes"):
        assert callable(getattr(B.BatchVerifier, name)), name
    hpp = open(os.path.join(ROOT, "include", "bpp_amd.hpp")).read()
    assert re.search(r"inline ScanResult scan_serialized_mixed_keys\(", hpp) and "bpp_range_scan_serialized_mixed_keys(" in hpp
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert "pub fn scan_serialized_mixed_keys(" in rs and "ffi::bpp_range_scan_serialized_mixed_keys(" in rs


def _device(L, v, pr, cm, pm, count, flags, keys, nk, idx, am, out, st, ws, wsb):
    return L.bpp_range_scan_serialized_mixed_keys_device(v, pr, cm, pm, count, flags, keys, nk, 5, idx, am, out, st, ws, wsb, None)


def _host(L, v, pr, cm, pm, count, flags, keys, nk, idx, am, out, st):
    return L.bpp_range_scan_serialized_mixed_keys(v, pr, cm, pm, count, flags, keys, nk, 5, idx, am, out, st)


def test_usage_errors_leave_the_buffers_alone():
    L = _lib()
    buf, pb = _bufs()
    eng = pb   # never read
    ms = np.array([1, 2, 4], dtype=np.uint32)
    pm = ms.ctypes.data_as(ctypes.c_void_p)
    T = TRANSCRIPT
    # a NULL engine, with work and without
    for count, nk in ((3, 2), (0, 2), (3, 0)):
        assert _device(L, None, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, pb, 1 << 20) == E_ARG and "null" in _err()
        assert _host(L, None, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb) == E_ARG and "null" in _err()
    # a NULL required pointer: proofs, commitments, m_of, keys, masks, status, workspace (index and amounts may be NULL)
    for i in range(7):
        a = [pb, pb, pm, pb, pb, pb, pb]
        a[i] = None
        assert _device(L, eng, a[0], a[1], a[2], 3, T, a[3], 2, None, None, a[4], a[5], a[6], 1 << 20) == E_ARG
        assert "null" in _err()
    for i in range(6):
        a = [pb, pb, pm, pb, pb, pb]
        a[i] = None
        assert _host(L, eng, a[0], a[1], a[2], 3, T, a[3], 2, None, None, a[4], a[5]) == E_ARG and "null" in _err()
    # keys without BPP_SER_TRANSCRIPT: they are the only blinding source, and blinding needs the transcript
    for fl in (0, UNCOMPRESSED, AMOUNT64, UNCOMPRESSED | AMOUNT64):
        assert _device(L, eng, pb, pb, pm, 3, fl, pb, 2, None, None, pb, pb, pb, 1 << 20) == E_ARG
        assert "BPP_SER_TRANSCRIPT" in _err()
        assert _host(L, eng, pb, pb, pm, 3, fl, pb, 2, None, None, pb, pb) == E_ARG and "BPP_SER_TRANSCRIPT" in _err()
    # unknown flags, also with nothing to do; the known ones pass the flag check
    for fl in (4, 8, 0x200, T | 4, AMOUNT64 | 4, -1):
        for count, nk in ((3, 2), (0, 2), (3, 0)):
            assert _device(L, eng, pb, pb, pm, count, fl, pb, nk, None, None, pb, pb, pb, 1 << 20) == E_ARG
            assert "unknown flag" in _err(), fl
            assert _host(L, eng, pb, pb, pm, count, fl, pb, nk, None, None, pb, pb) == E_ARG and "unknown flag" in _err()
    for fl in (T, T | UNCOMPRESSED, T | AMOUNT64, T | UNCOMPRESSED | AMOUNT64):
        assert _device(L, eng, None, None, pm, 3, fl, pb, 2, None, None, pb, pb, pb, 1 << 20) == E_ARG
        assert "null" in _err() and "unknown flag" not in _err(), hex(fl)
    # an m_i no engine takes: the text names i
    for bad, at in (([1, 3, 2], 1), ([0, 1, 1], 0), ([2, 4, 12], 2)):
        b = np.array(bad, dtype=np.uint32)
        pbad = b.ctypes.data_as(ctypes.c_void_p)
        assert _device(L, eng, pb, pb, pbad, 3, T, pb, 2, None, None, pb, pb, pb, 1 << 20) == E_ARG and "m_of[%d]" % at in _err()
        assert _host(L, eng, pb, pb, pbad, 3, T, pb, 2, None, None, pb, pb) == E_ARG and "m_of[%d]" % at in _err()
        assert L.bpp_scan_serialized_mixed_keys_workspace_bytes(eng, pbad, 3, 2) == 0
    # n_keys x count over the bound of the other entries' count: just over it, each factor alone over it, and products
    # that wrap 64 bits (to 0, and to 3)
    assert BOUND // 3 * 3 <= BOUND < (BOUND // 3 + 1) * 3
    for count, nk in ((3, BOUND // 3 + 1), (3, BOUND + 1), (3, 1 << 62), (3, (1 << 64) // 3 + 1), (2, 1 << 63), (3, (1 << 64) - 1)):
        assert _device(L, eng, pb, pb, pm, count, T, pb, nk, None, None, pb, pb, pb, 1 << 20) == E_ARG
        assert "n_keys x count too large" in _err(), (count, nk)
        assert _host(L, eng, pb, pb, pm, count, T, pb, nk, None, None, pb, pb) == E_ARG and "n_keys x count too large" in _err()
        assert L.bpp_scan_serialized_mixed_keys_workspace_bytes(eng, pm, count, nk) == 0
    # keys that are not word-aligned; a workspace of no bytes
    odd = ctypes.c_void_p(pb.value + 1)
    assert _device(L, eng, pb, pb, pm, 3, T, odd, 2, None, None, pb, pb, pb, 1 << 20) == E_ARG and "aligned" in _err()
    assert _device(L, eng, pb, pb, pm, 3, T, pb, 2, None, None, pb, pb, pb, 0) == E_ARG and "workspace too small" in _err()
    # n_keys = 0 or count = 0 is BPP_OK, whatever else is NULL
    for count, nk in ((0, 2), (3, 0), (0, 0)):
        assert _device(L, eng, None, None, None, count, T, None, nk, None, None, None, None, None, 0) == 0
        assert _host(L, eng, None, None, None, count, T | AMOUNT64, None, nk, None, None, None, None) == 0
    assert L.bpp_scan_serialized_mixed_keys_workspace_bytes(None, pm, 3, 2) == 0
    assert L.bpp_scan_serialized_mixed_keys_workspace_bytes(eng, None, 3, 2) == 0
    assert buf.tolist() == [0x77] * 64   # nothing was written
