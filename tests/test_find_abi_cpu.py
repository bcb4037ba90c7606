"""CPU: the fused verify-and-find entry points and the sealing calls (bpp_verify_find_serialized_mixed_keys_workspace_bytes,
bpp_range_verify_find_serialized_mixed_keys[_device], bpp_amounts_seal[_device]) are declared, exported, bound and present
in the Rust FFI; they run under the entry shim; the Python, C++ and Rust wrappers exist; their usage errors are BPP_E_ARG and
leave the caller's buffers alone.  No GPU needed: every case here is answered by an argument check before the engine handle
is read, so a dummy non-null handle stands in for one.  The cases that need the engine -- a workspace smaller than the
layout, a call with nothing to do -- are in tests/test_gpu_find.py."""

import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIND = ("bpp_verify_find_serialized_mixed_keys_workspace_bytes", "bpp_range_verify_find_serialized_mixed_keys_device",
        "bpp_range_verify_find_serialized_mixed_keys")
SEAL = ("bpp_amounts_seal_device", "bpp_amounts_seal")
TRANSCRIPT, UNCOMPRESSED, AMOUNT64, SEALED = 1, 2, 0x100, 0x200
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
    for s in FIND + SEAL:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in M.EXPORTS, s
        assert hasattr(L, s), s
        assert "pub fn %s(" % s in ffi, s
    assert re.search(r"#define BPP_FIND_AMOUNTS_SEALED 0x200\b", hdr)
    # the header says what a hit is, gives the order and the overflow rule, and that this call IS a verification
    block = raw[raw.index("VERIFY a block and LIST"):raw.index("size_t bpp_verify_find_serialized_mixed_keys_workspace_bytes(")]
    for text in ("THIS CALL IS A VERIFICATION OF THE BLOCK", "A HIT IMPLIES A VERIFIED PROOF", "VIEW KEY",
                 "IN ASCENDING (key number, caller position) ORDER", "nothing beyond min(n_hits, max_hits) records is touched",
                 "SHARED BY ALL KEYS", "overwrites that buffer before freeing it", "BPP_SER_TRANSCRIPT (REQUIRED",
                 "no dense status matrix"):
        assert text in block, text
    seal = raw[raw.index("sealed amounts: the 8-byte ciphertext"):raw.index("int bpp_amounts_seal_device(")]
    for text in ('"bppa"', "THE INDEX RULE ABOVE HOLDS UNCHANGED", "Sealing and opening are the same operation"):
        assert text in seal, text


def test_entries_run_under_the_guard():
    import test_abi_guard_cpu as G
    entries = G._entry_points(open(os.path.join(ROOT, "bulletproofsplus_amd", "csrc", "capi.hip")).read())
    for s in FIND + SEAL:
        assert s in entries and any(shim in entries[s] for shim in G.SHIMS), s
        if "workspace_bytes" not in s:
            assert '{count, "count"}' in entries[s], (s, "count is not bounded by the shim")
    for s in FIND[1:]:
        assert "find_args(" in entries[s] and "pairs_bounded(a.n_keys, pair_units(" in G._receiver_check("find_args"), \
            (s, "n_keys x count is not bounded before the engine is read")


def test_wrappers_exist():
    import bulletproofsplus_amd as B
    for name in ("seal_amounts", "seal_amounts_device", "verify_find_serialized_mixed_keys",
                 "verify_find_serialized_mixed_keys_device", "verify_find_workspace_bytes"):
        assert callable(getattr(B.BatchVerifier, name)), name
    hpp = open(os.path.join(ROOT, "include", "bpp_amd.hpp")).read()
    assert re.search(r"inline FindResult verify_find_serialized_mixed_keys\(", hpp)
    assert "bpp_range_verify_find_serialized_mixed_keys(" in hpp and "bpp_amounts_seal(" in hpp
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert "pub fn verify_find_serialized_mixed_keys(" in rs and "ffi::bpp_range_verify_find_serialized_mixed_keys(" in rs
    assert "pub fn seal_amounts(" in rs and "ffi::bpp_amounts_seal(" in rs


def _device(L, v, pr, cm, pm, count, flags, keys, nk, idx, am, ok, hits, max_hits, nh, ws, wsb):
    return L.bpp_range_verify_find_serialized_mixed_keys_device(v, pr, cm, pm, count, flags, keys, nk, 5, idx, am, ok, hits,
                                                                max_hits, nh, ws, wsb, None)


def _host(L, v, pr, cm, pm, count, flags, keys, nk, idx, am, ok, hits, max_hits, nh):
    return L.bpp_range_verify_find_serialized_mixed_keys(v, pr, cm, pm, count, flags, keys, nk, 5, idx, am, ok, hits, max_hits, nh)


def test_usage_errors_leave_the_buffers_alone():
    L = _lib()
    buf, pb = _bufs()
    eng = pb   # never read
    ms = np.array([1, 2, 4], dtype=np.uint32)
    pm = ms.ctypes.data_as(ctypes.c_void_p)
    T = TRANSCRIPT
    # a NULL engine, with work and without
    for count, nk in ((3, 2), (0, 2), (3, 0)):
        assert _device(L, None, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, 4, pb, pb, 1 << 20) == E_ARG and "null" in _err()
        assert _host(L, None, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, 4, pb) == E_ARG and "null" in _err()
    # a NULL required pointer: proofs, commitments, m_of, keys, amounts, verdicts, hit records (max_hits > 0), the count of
    # hits, workspace (the index may be NULL); without keys the block is still verified, so the pointers the
    # verification needs stay required
    for i in range(9):
        a = [pb, pb, pm, pb, pb, pb, pb, pb, pb]
        a[i] = None
        assert _device(L, eng, a[0], a[1], a[2], 3, T, a[3], 2, None, a[4], a[5], a[6], 4, a[7], a[8], 1 << 20) == E_ARG
        assert "null" in _err(), i
    for i in range(8):
        a = [pb, pb, pm, pb, pb, pb, pb, pb]
        a[i] = None
        assert _host(L, eng, a[0], a[1], a[2], 3, T, a[3], 2, None, a[4], a[5], a[6], 4, a[7]) == E_ARG and "null" in _err(), i
    for i in (0, 1, 2, 5, 7, 8):
        a = [pb, pb, pm, None, None, pb, None, pb, pb]
        a[i] = None
        assert _device(L, eng, a[0], a[1], a[2], 3, T, a[3], 0, None, a[4], a[5], a[6], 4, a[7], a[8], 1 << 20) == E_ARG
        assert "null" in _err(), i
    for i in (0, 1, 2, 5, 7):
        a = [pb, pb, pm, None, None, pb, None, pb]
        a[i] = None
        assert _host(L, eng, a[0], a[1], a[2], 3, T, a[3], 0, None, a[4], a[5], a[6], 4, a[7]) == E_ARG and "null" in _err(), i
    # the count of hits is required even with nothing to do
    for count, nk in ((0, 2), (3, 0)):
        assert _device(L, eng, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, 4, None, pb, 1 << 20) == E_ARG and "null" in _err()
        assert _host(L, eng, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, 4, None) == E_ARG and "null" in _err()
    # keys without BPP_SER_TRANSCRIPT
    for fl in (0, UNCOMPRESSED, AMOUNT64, SEALED, UNCOMPRESSED | AMOUNT64 | SEALED):
        assert _device(L, eng, pb, pb, pm, 3, fl, pb, 2, None, pb, pb, pb, 4, pb, pb, 1 << 20) == E_ARG
        assert "BPP_SER_TRANSCRIPT" in _err()
        assert _host(L, eng, pb, pb, pm, 3, fl, pb, 2, None, pb, pb, pb, 4, pb) == E_ARG and "BPP_SER_TRANSCRIPT" in _err()
    # unknown flags, also with nothing to do; the known ones pass the flag check
    for fl in (4, 8, 0x400, T | 4, SEALED | 0x80, -1):
        for count, nk in ((3, 2), (0, 2), (3, 0)):
            assert _device(L, eng, pb, pb, pm, count, fl, pb, nk, None, pb, pb, pb, 4, pb, pb, 1 << 20) == E_ARG
            assert "unknown flag" in _err(), fl
            assert _host(L, eng, pb, pb, pm, count, fl, pb, nk, None, pb, pb, pb, 4, pb) == E_ARG and "unknown flag" in _err()
    for fl in (T, T | SEALED, T | UNCOMPRESSED | AMOUNT64 | SEALED):
        assert _device(L, eng, None, None, pm, 3, fl, pb, 2, None, pb, pb, pb, 4, pb, pb, 1 << 20) == E_ARG
        assert "null" in _err() and "unknown flag" not in _err(), hex(fl)
    # an m_i no engine takes: the text names i
    for bad, at in (([1, 3, 2], 1), ([0, 1, 1], 0), ([2, 4, 12], 2)):
        b = np.array(bad, dtype=np.uint32)
        pbad = b.ctypes.data_as(ctypes.c_void_p)
        assert _device(L, eng, pb, pb, pbad, 3, T, pb, 2, None, pb, pb, pb, 4, pb, pb, 1 << 20) == E_ARG
        assert "m_of[%d]" % at in _err()
        assert _host(L, eng, pb, pb, pbad, 3, T, pb, 2, None, pb, pb, pb, 4, pb) == E_ARG and "m_of[%d]" % at in _err()
        assert L.bpp_verify_find_serialized_mixed_keys_workspace_bytes(eng, pbad, 3, 2) == 0
    # n_keys x count over the bound: just over it, each factor alone over it, and products that wrap 64 bits
    for count, nk in ((3, BOUND // 3 + 1), (3, BOUND + 1), (3, 1 << 62), (3, (1 << 64) // 3 + 1), (2, 1 << 63), (3, (1 << 64) - 1)):
        assert _device(L, eng, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, 4, pb, pb, 1 << 20) == E_ARG
        assert "n_keys x count too large" in _err(), (count, nk)
        assert _host(L, eng, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, 4, pb) == E_ARG and "n_keys x count too large" in _err()
        assert L.bpp_verify_find_serialized_mixed_keys_workspace_bytes(eng, pm, count, nk) == 0
    # keys that are not word-aligned; a workspace of no bytes
    odd = ctypes.c_void_p(pb.value + 1)
    assert _device(L, eng, pb, pb, pm, 3, T, odd, 2, None, pb, pb, pb, 4, pb, pb, 1 << 20) == E_ARG and "aligned" in _err()
    assert _device(L, eng, pb, pb, pm, 3, T, pb, 2, None, pb, pb, pb, 4, pb, pb, 0) == E_ARG and "workspace too small" in _err()
    # the host twin with no proof: BPP_OK and a count of zero, whatever else is NULL
    for count, nk in ((0, 2), (0, 0)):
        n = np.full(1, 0x77, dtype=np.uint32)
        assert _host(L, eng, None, None, None, count, T | SEALED, None, nk, None, None, None, None, 0,
                     n.ctypes.data_as(ctypes.c_void_p)) == 0
        assert n[0] == 0
    # the size function returns 0 where its sibling does
    assert L.bpp_verify_find_serialized_mixed_keys_workspace_bytes(None, pm, 3, 2) == 0
    assert L.bpp_verify_find_serialized_mixed_keys_workspace_bytes(eng, None, 3, 2) == 0
    assert L.bpp_scan_serialized_mixed_keys_workspace_bytes(None, pm, 3, 2) == 0
    assert L.bpp_scan_serialized_mixed_keys_workspace_bytes(eng, None, 3, 2) == 0
    assert buf.tolist() == [0x77] * 64   # nothing was written


def test_sealing_usage_errors():
    L = _lib()
    buf, pb = _bufs()
    key = bytes(32)
    for ctx, k, i, o in ((None, key, pb, pb), (pb, None, pb, pb), (pb, key, None, pb), (pb, key, pb, None)):
        assert L.bpp_amounts_seal_device(ctx, k, 0, None, i, 3, o, None) == E_ARG and "null" in _err()
        assert L.bpp_amounts_seal(ctx, k, 0, None, i, 3, o) == E_ARG and "null" in _err()
    for count in (BOUND + 1, 1 << 32, 1 << 63):
        assert L.bpp_amounts_seal_device(pb, key, 0, None, pb, count, pb, None) == E_ARG and "too large" in _err()
        assert L.bpp_amounts_seal(pb, key, 0, None, pb, count, pb) == E_ARG and "too large" in _err()
    assert L.bpp_amounts_seal_device(pb, key, 0, None, None, 0, None, None) == 0
    assert L.bpp_amounts_seal(pb, key, 0, None, None, 0, None) == 0
    assert buf.tolist() == [0x77] * 64
