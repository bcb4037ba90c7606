"""CPU: the view-tag calls and the tagged verify-and-find entry points (bpp_view_tags[_device],
bpp_verify_find_tagged_workspace_bytes, bpp_range_verify_find_tagged_serialized_mixed_keys[_device]) are declared, exported,
bound and present in the Rust FFI; they run under the entry shim; the Python, C++ and Rust wrappers exist; their usage
errors are BPP_E_ARG and leave the caller's buffers alone.  No GPU needed: every case here is answered by an argument check
before the engine handle is read, so a dummy non-null handle stands in for one.  The cases that need the engine -- a
workspace one byte short, an m_i above the engine's, calls with nothing to do -- are in tests/test_gpu_find_tags.py."""

import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGGED = ("bpp_verify_find_tagged_workspace_bytes", "bpp_range_verify_find_tagged_serialized_mixed_keys_device",
          "bpp_range_verify_find_tagged_serialized_mixed_keys")
TAGS = ("bpp_view_tags_device", "bpp_view_tags")
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
    for s in TAGGED + TAGS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in M.EXPORTS, s
        assert hasattr(L, s), s
        assert "pub fn %s(" % s in ffi, s
    # the header defines the tag, says who makes it and that it authenticates nothing
    tags = raw[raw.index("view tags: the one byte an output carries"):raw.index("int bpp_view_tags_device(")]
    for text in ('"bppt"', "the first byte of SHA-256(key ||", "THE SENDER MAKES THE TAG", "IT DOES NOT AUTHENTICATE ANYTHING",
                 "THE INDEX RULE ABOVE HOLDS UNCHANGED", "exactly as a wrong sealed", "count = 0 is BPP_OK"):
        assert text in tags, text
    # the tagged call: what a candidate is, that the verdicts and the hits are the untagged call's, the key rule, no sync
    block = raw[raw.index("TESTING THE VIEW TAGS FIRST"):raw.index("size_t bpp_verify_find_tagged_workspace_bytes(")]
    for text in ("d_ok IS EXACTLY THE UNTAGGED CALL'S", "A CANDIDATE is a pair", "view_tag(key_j, index_i) == d_tags[i]",
                 "A HIT IS A CANDIDATE THAT IS A HIT OF THE UNTAGGED CALL", "SHARED BY ALL KEYS", "REQUIRED when n_keys > 0",
                 "may be NULL", "the candidate bit", "BLOCKS the host only while it uploads the per-proof index",
                 "THE BLOCK VERIFIED ALL THE SAME", "room for every pair being a candidate"):
        assert text in block, text
    # the untagged declarations are where they were: this work adds, it changes nothing
    assert "int bpp_range_verify_find_serialized_mixed_keys_device(bpp_verifier *v, const void *d_proofs" in raw


def test_entries_run_under_the_guard():
    import test_abi_guard_cpu as G
    entries = G._entry_points(open(os.path.join(ROOT, "bulletproofsplus_amd", "csrc", "capi.hip")).read())
    for s in TAGGED + TAGS:
        assert s in entries and any(shim in entries[s] for shim in G.SHIMS), s
        if "workspace_bytes" not in s:
            assert '{count, "count"}' in entries[s], (s, "count is not bounded by the shim")
    for s in TAGGED[1:]:
        assert "find_args(" in entries[s] and "pairs_bounded(a.n_keys, pair_units(" in G._receiver_check("find_args"), \
            (s, "n_keys x count is not bounded before the engine is read")
    assert "pairs_bounded(" in entries[TAGGED[0]]


def test_wrappers_exist():
    import inspect

    import bulletproofsplus_amd as B
    for name in ("view_tags", "view_tags_device", "verify_find_tagged_workspace_bytes"):
        assert callable(getattr(B.BatchVerifier, name)), name
    assert "tags" in inspect.signature(B.BatchVerifier.verify_find_serialized_mixed_keys).parameters
    dev = inspect.signature(B.BatchVerifier.verify_find_serialized_mixed_keys_device).parameters
    assert "d_tags" in dev and "d_n_candidates" in dev
    hpp = open(os.path.join(ROOT, "include", "bpp_amd.hpp")).read()
    assert re.search(r"inline FindTaggedResult verify_find_tagged_serialized_mixed_keys\(", hpp)
    assert "bpp_range_verify_find_tagged_serialized_mixed_keys(" in hpp and "bpp_view_tags(" in hpp
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert "pub fn verify_find_tagged_serialized_mixed_keys(" in rs
    assert "ffi::bpp_range_verify_find_tagged_serialized_mixed_keys(" in rs
    assert "pub fn view_tags(" in rs and "ffi::bpp_view_tags(" in rs


def _device(L, v, pr, cm, pm, count, flags, keys, nk, idx, am, ok, hits, max_hits, nh, tags, nc, ws, wsb):
    return L.bpp_range_verify_find_tagged_serialized_mixed_keys_device(v, pr, cm, pm, count, flags, keys, nk, 5, idx, am, ok, hits,
                                                                       max_hits, nh, tags, nc, ws, wsb, None)


def _host(L, v, pr, cm, pm, count, flags, keys, nk, idx, am, ok, hits, max_hits, nh, tags, nc):
    return L.bpp_range_verify_find_tagged_serialized_mixed_keys(v, pr, cm, pm, count, flags, keys, nk, 5, idx, am, ok, hits,
                                                                max_hits, nh, tags, nc)


def test_usage_errors_leave_the_buffers_alone():
    L = _lib()
    buf, pb = _bufs()
    eng = pb   # never read
    ms = np.array([1, 2, 4], dtype=np.uint32)
    pm = ms.ctypes.data_as(ctypes.c_void_p)
    T = TRANSCRIPT
    # a NULL engine, with work and without
    for count, nk in ((3, 2), (0, 2), (3, 0)):
        assert _device(L, None, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, 4, pb, pb, pb, pb, 1 << 20) == E_ARG
        assert "null" in _err()
        assert _host(L, None, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, 4, pb, pb, pb) == E_ARG and "null" in _err()
    # NULL d_tags with keys: an error; so is every pointer the untagged call requires.  d_n_candidates may be NULL: with
    # it NULL and everything else in place the call gets past the pointer checks (and fails on the next one, the flags)
    for i in range(10):
        a = [pb, pb, pm, pb, pb, pb, pb, pb, pb, pb]   # proofs, commitments, m_of, keys, amounts, ok, hits, n_hits, tags, ws
        a[i] = None
        assert _device(L, eng, a[0], a[1], a[2], 3, T, a[3], 2, None, a[4], a[5], a[6], 4, a[7], a[8], pb, a[9], 1 << 20) == E_ARG
        assert "null" in _err(), i
    for i in range(9):
        a = [pb, pb, pm, pb, pb, pb, pb, pb, pb]
        a[i] = None
        assert _host(L, eng, a[0], a[1], a[2], 3, T, a[3], 2, None, a[4], a[5], a[6], 4, a[7], a[8], pb) == E_ARG
        assert "null" in _err(), i
    assert _device(L, eng, pb, pb, pm, 3, 0, pb, 2, None, pb, pb, pb, 4, pb, pb, None, pb, 1 << 20) == E_ARG
    assert "BPP_SER_TRANSCRIPT" in _err()
    assert _host(L, eng, pb, pb, pm, 3, 0, pb, 2, None, pb, pb, pb, 4, pb, pb, None) == E_ARG and "BPP_SER_TRANSCRIPT" in _err()
    # without keys the tags are not required, the pointers of the verification are
    for i in (0, 1, 2, 5, 7, 9):
        a = [pb, pb, pm, None, None, pb, None, pb, None, pb]
        a[i] = None
        assert _device(L, eng, a[0], a[1], a[2], 3, T, a[3], 0, None, a[4], a[5], a[6], 4, a[7], a[8], None, a[9], 1 << 20) == E_ARG
        assert "null" in _err(), i
    assert _device(L, eng, pb, pb, pm, 3, 0, None, 0, None, None, pb, None, 4, pb, None, None, pb, 1 << 20) == E_ARG
    assert "BPP_SER_TRANSCRIPT" in _err()   # past the pointer checks with d_tags NULL and no keys
    # the count of hits is required even with nothing to do
    for count, nk in ((0, 2), (3, 0)):
        assert _device(L, eng, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, 4, None, pb, pb, pb, 1 << 20) == E_ARG
        assert "null" in _err()
        assert _host(L, eng, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, 4, None, pb, pb) == E_ARG and "null" in _err()
    # unknown flags, also with nothing to do
    for fl in (4, 8, 0x400, T | 4, SEALED | 0x80, -1):
        for count, nk in ((3, 2), (0, 2), (3, 0)):
            assert _device(L, eng, pb, pb, pm, count, fl, pb, nk, None, pb, pb, pb, 4, pb, pb, pb, pb, 1 << 20) == E_ARG
            assert "unknown flag" in _err(), fl
            assert _host(L, eng, pb, pb, pm, count, fl, pb, nk, None, pb, pb, pb, 4, pb, pb, pb) == E_ARG
            assert "unknown flag" in _err(), fl
    # an m_i no engine takes: the text names i
    for bad, at in (([1, 3, 2], 1), ([0, 1, 1], 0), ([2, 4, 12], 2)):
        b = np.array(bad, dtype=np.uint32)
        pbad = b.ctypes.data_as(ctypes.c_void_p)
        assert _device(L, eng, pb, pb, pbad, 3, T, pb, 2, None, pb, pb, pb, 4, pb, pb, pb, pb, 1 << 20) == E_ARG
        assert "m_of[%d]" % at in _err()
        assert _host(L, eng, pb, pb, pbad, 3, T, pb, 2, None, pb, pb, pb, 4, pb, pb, pb) == E_ARG and "m_of[%d]" % at in _err()
        assert L.bpp_verify_find_tagged_workspace_bytes(eng, pbad, 3, 2) == 0
        assert L.bpp_verify_find_serialized_mixed_keys_workspace_bytes(eng, pbad, 3, 2) == 0
    # n_keys x count over the bound: just over it, each factor alone over it, and products that wrap 64 bits
    for count, nk in ((3, BOUND // 3 + 1), (3, BOUND + 1), (3, 1 << 62), (3, (1 << 64) // 3 + 1), (2, 1 << 63), (3, (1 << 64) - 1)):
        assert _device(L, eng, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, 4, pb, pb, pb, pb, 1 << 20) == E_ARG
        assert "n_keys x count too large" in _err(), (count, nk)
        assert _host(L, eng, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, 4, pb, pb, pb) == E_ARG
        assert "n_keys x count too large" in _err(), (count, nk)
        assert L.bpp_verify_find_tagged_workspace_bytes(eng, pm, count, nk) == 0
        assert L.bpp_verify_find_serialized_mixed_keys_workspace_bytes(eng, pm, count, nk) == 0
    # keys that are not word-aligned; a workspace of no bytes (a short one needs the engine: tests/test_gpu_find_tags.py)
    odd = ctypes.c_void_p(pb.value + 1)
    assert _device(L, eng, pb, pb, pm, 3, T, odd, 2, None, pb, pb, pb, 4, pb, pb, pb, pb, 1 << 20) == E_ARG and "aligned" in _err()
    assert _device(L, eng, pb, pb, pm, 3, T, pb, 2, None, pb, pb, pb, 4, pb, pb, pb, pb, 0) == E_ARG
    assert "workspace too small" in _err()
    # the host twin with no proof: BPP_OK, no hit and no candidate, whatever else is NULL
    for count, nk in ((0, 2), (0, 0)):
        n = np.full(2, 0x77, dtype=np.uint32)
        assert _host(L, eng, None, None, None, count, T | SEALED, None, nk, None, None, None, None, 0,
                     n[:1].ctypes.data_as(ctypes.c_void_p), None, n[1:].ctypes.data_as(ctypes.c_void_p)) == 0
        assert n.tolist() == [0, 0]
        n[:] = 0x77
        assert _host(L, eng, None, None, None, count, T, None, nk, None, None, None, None, 0,
                     n[:1].ctypes.data_as(ctypes.c_void_p), None, None) == 0
        assert n.tolist() == [0, 0x77]
    # the size function returns 0 where the untagged one does
    for v, m in ((None, pm), (eng, None)):
        assert L.bpp_verify_find_tagged_workspace_bytes(v, m, 3, 2) == 0
        assert L.bpp_verify_find_serialized_mixed_keys_workspace_bytes(v, m, 3, 2) == 0
    assert buf.tolist() == [0x77] * 64   # nothing was written


def test_tag_making_usage_errors():
    L = _lib()
    buf, pb = _bufs()
    key = bytes(32)
    for ctx, k, o in ((None, key, pb), (pb, None, pb), (pb, key, None)):
        assert L.bpp_view_tags_device(ctx, k, 0, None, 3, o, None) == E_ARG and "null" in _err()
        assert L.bpp_view_tags(ctx, k, 0, None, 3, o) == E_ARG and "null" in _err()
    for count in (BOUND + 1, 1 << 32, 1 << 63):
        assert L.bpp_view_tags_device(pb, key, 0, None, count, pb, None) == E_ARG and "too large" in _err()
        assert L.bpp_view_tags(pb, key, 0, None, count, pb) == E_ARG and "too large" in _err()
    assert L.bpp_view_tags_device(pb, key, 0, None, 0, None, None) == 0
    assert L.bpp_view_tags(pb, key, 0, None, 0, None) == 0
    assert buf.tolist() == [0x77] * 64
