"""CPU: the calls for outputs with derived masks (bpp_outputs_make[_device], bpp_verify_find_outputs_workspace_bytes,
bpp_range_verify_find_outputs_serialized_mixed_keys[_device]) are declared, exported, bound and present in the Rust FFI;
they run under the entry shim; the Python, C++ and Rust wrappers exist; their usage errors are BPP_E_ARG and leave the
caller's buffers alone.  No GPU needed: every case here is answered by an argument check before the engine handle is read,
so a dummy non-null handle stands in for one.  The cases that need the engine -- a workspace one byte short, an m_i above
the engine's, calls with nothing to do -- are in tests/test_gpu_outputs.py."""

import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIND = ("bpp_verify_find_outputs_workspace_bytes", "bpp_range_verify_find_outputs_serialized_mixed_keys_device",
        "bpp_range_verify_find_outputs_serialized_mixed_keys")
MAKE = ("bpp_outputs_make_device", "bpp_outputs_make")
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
    for s in FIND + MAKE:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in M.EXPORTS, s
        assert hasattr(L, s), s
        assert "pub fn %s(" % s in ffi, s
    # the section sits after the tagged call's prototypes and before the seam
    at = raw.index("outputs with DERIVED masks")
    assert raw.index("int bpp_range_verify_find_tagged_serialized_mixed_keys(") < at < raw.index("the weighted inner product argument")
    block = re.sub(r"[\s*]+", " ", raw[at:raw.index("the weighted inner product argument")])   # line breaks do not count
    for text in ('"bppm"', '"bppa"', '"bppt"', "(c0 + 2^256 c1) mod r, zero replaced by one", "the first 8 bytes of B(",
                 "the first byte of B(", "SHA-256(key || tag (4 ASCII bytes) || idx as u64 LE || a as u32 LE || b as u32 LE)",
                 "FOR j = 0 THE PAD AND THE TAG ARE BYTE FOR BYTE", "a valid output here",
                 "THE INDEX RULE ABOVE HOLDS UNCHANGED", "never meets the same (idx, j) twice", "A MASK IS SECRET",
                 "whoever holds (key, idx, j) holds the mask", "A CANDIDATE is a pair",
                 "output_tag(key_q, idx_i, j) == d_tags[o]", "A HIT is a candidate with", "V_{i,j} == v g + gamma h",
                 "FOR EVERY m_i", "A HIT IMPLIES", "A VERIFIED PROOF", "THE KEY RULE", "uses LDS or scratch",
                 "A non-hit's mask never leaves registers", "BPP_FIND_AMOUNTS_SEALED is NOT", "SHARED BY ALL KEYS",
                 "REQUIRED when n_keys > 0", "THE BLOCK VERIFIED ALL THE SAME", "checked without overflow",
                 "BLOCKS the host only while it uploads the per-proof index"):
        assert text in block, text
    assert "A HIT IMPLIES A VERIFIED PROOF" in block
    # the existing declarations are where they were: this work adds, it changes nothing
    assert "Aggregated proofs (m_i > 1) are verified and never listed" in raw
    assert "int bpp_range_verify_find_tagged_serialized_mixed_keys_device(bpp_verifier *v, const void *d_proofs" in raw


def test_entries_run_under_the_guard():
    import test_abi_guard_cpu as G
    entries = G._entry_points(open(os.path.join(ROOT, "bulletproofsplus_amd", "csrc", "capi.hip")).read())
    for s in FIND + MAKE:
        assert s in entries and any(shim in entries[s] for shim in G.SHIMS), s
    for s in FIND[1:]:
        assert '{count, "count"}' in entries[s], (s, "count is not bounded by the shim")
        assert "FIND_PER_OUTPUT" in entries[s] and "find_args(" in entries[s], s
        check = G._receiver_check("find_args")
        assert "per_output = a.mode == FIND_PER_OUTPUT" in check and "pair_units(units_of, a.count, per_output)" in check, \
            (s, "n_keys x n_out is not bounded before the engine is read")
    for s in MAKE:
        assert '{n_out, "n_out"}' in entries[s], s
    assert "pairs_bounded(n_keys, pair_units(m_of, count, true))" in entries[FIND[0]]


def test_wrappers_exist():
    import inspect

    import bulletproofsplus_amd as B
    for name in ("make_outputs", "make_outputs_device", "verify_find_outputs_workspace_bytes",
                 "verify_find_outputs_serialized_mixed_keys", "verify_find_outputs_serialized_mixed_keys_device"):
        assert callable(getattr(B.BatchVerifier, name)), name
    sig = inspect.signature(B.BatchVerifier.make_outputs).parameters
    assert list(sig)[1:] == ["keys", "amounts", "ms", "index_base", "index"]
    hpp = open(os.path.join(ROOT, "include", "bpp_amd.hpp")).read()
    assert re.search(r"inline FindTaggedResult verify_find_outputs_serialized_mixed_keys\(", hpp)
    assert "bpp_range_verify_find_outputs_serialized_mixed_keys(" in hpp and "bpp_outputs_make(" in hpp
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert "pub fn verify_find_outputs_serialized_mixed_keys(" in rs
    assert "ffi::bpp_range_verify_find_outputs_serialized_mixed_keys(" in rs
    assert "pub fn make_outputs(" in rs and "ffi::bpp_outputs_make(" in rs


def _device(L, v, pr, cm, pm, count, flags, keys, nk, idx, se, tg, ok, hits, max_hits, nh, nc, ws, wsb):
    return L.bpp_range_verify_find_outputs_serialized_mixed_keys_device(v, pr, cm, pm, count, flags, keys, nk, 5, idx, se, tg, ok,
                                                                        hits, max_hits, nh, nc, ws, wsb, None)


def _host(L, v, pr, cm, pm, count, flags, keys, nk, idx, se, tg, ok, hits, max_hits, nh, nc):
    return L.bpp_range_verify_find_outputs_serialized_mixed_keys(v, pr, cm, pm, count, flags, keys, nk, 5, idx, se, tg, ok, hits,
                                                                 max_hits, nh, nc)


def test_usage_errors_leave_the_buffers_alone():
    L = _lib()
    buf, pb = _bufs()
    eng = pb   # never read
    ms = np.array([1, 2, 4], dtype=np.uint32)   # 7 outputs
    pm = ms.ctypes.data_as(ctypes.c_void_p)
    T = TRANSCRIPT
    # a NULL engine, with work and without
    for count, nk in ((3, 2), (0, 2), (3, 0)):
        assert _device(L, None, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, pb, 4, pb, pb, pb, 1 << 20) == E_ARG
        assert "null" in _err()
        assert _host(L, None, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, pb, 4, pb, pb) == E_ARG and "null" in _err()
    # every required pointer; d_n_candidates may be NULL: with it NULL and everything else in place the call gets past the
    # pointer checks (and fails on the next one, the flags)
    for i in range(10):
        a = [pb, pb, pm, pb, pb, pb, pb, pb, pb, pb]   # proofs, commitments, m_of, keys, sealed, tags, ok, hits, n_hits, ws
        a[i] = None
        assert _device(L, eng, a[0], a[1], a[2], 3, T, a[3], 2, None, a[4], a[5], a[6], a[7], 4, a[8], pb, a[9], 1 << 20) == E_ARG
        assert "null" in _err(), i
    for i in range(9):
        a = [pb, pb, pm, pb, pb, pb, pb, pb, pb]
        a[i] = None
        assert _host(L, eng, a[0], a[1], a[2], 3, T, a[3], 2, None, a[4], a[5], a[6], a[7], 4, a[8], pb) == E_ARG
        assert "null" in _err(), i
    assert _device(L, eng, pb, pb, pm, 3, 0, pb, 2, None, pb, pb, pb, pb, 4, pb, None, pb, 1 << 20) == E_ARG
    assert "BPP_SER_TRANSCRIPT" in _err()
    assert _host(L, eng, pb, pb, pm, 3, 0, pb, 2, None, pb, pb, pb, pb, 4, pb, None) == E_ARG and "BPP_SER_TRANSCRIPT" in _err()
    # without keys the sealed amounts and the tags are not required, the pointers of the verification are
    for i in (0, 1, 2, 6, 8, 9):
        a = [pb, pb, pm, None, None, None, pb, None, pb, pb]
        a[i] = None
        assert _device(L, eng, a[0], a[1], a[2], 3, T, a[3], 0, None, a[4], a[5], a[6], a[7], 4, a[8], None, a[9], 1 << 20) == E_ARG
        assert "null" in _err(), i
    assert _device(L, eng, pb, pb, pm, 3, 0, None, 0, None, None, None, pb, None, 4, pb, None, pb, 1 << 20) == E_ARG
    assert "BPP_SER_TRANSCRIPT" in _err()   # past the pointer checks with no keys
    # the count of hits is required even with nothing to do
    for count, nk in ((0, 2), (3, 0)):
        assert _device(L, eng, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, pb, 4, None, pb, pb, 1 << 20) == E_ARG
        assert "null" in _err()
        assert _host(L, eng, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, pb, 4, None, pb) == E_ARG and "null" in _err()
    # the sealed flag is not taken; unknown flags; also with nothing to do
    for fl, text in ((T | SEALED, "BPP_FIND_AMOUNTS_SEALED"), (SEALED, "BPP_FIND_AMOUNTS_SEALED"), (4, "unknown flag"),
                     (8, "unknown flag"), (0x400, "unknown flag"), (T | 4, "unknown flag"), (T | 0x80, "unknown flag")):
        for count, nk in ((3, 2), (0, 2), (3, 0)):
            assert _device(L, eng, pb, pb, pm, count, fl, pb, nk, None, pb, pb, pb, pb, 4, pb, pb, pb, 1 << 20) == E_ARG
            assert text in _err(), fl
            assert _host(L, eng, pb, pb, pm, count, fl, pb, nk, None, pb, pb, pb, pb, 4, pb, pb) == E_ARG
            assert text in _err(), fl
    # an m_i no engine takes: the text names i
    for bad, at in (([1, 3, 2], 1), ([0, 1, 1], 0), ([2, 4, 12], 2)):
        b = np.array(bad, dtype=np.uint32)
        pbad = b.ctypes.data_as(ctypes.c_void_p)
        assert _device(L, eng, pb, pb, pbad, 3, T, pb, 2, None, pb, pb, pb, pb, 4, pb, pb, pb, 1 << 20) == E_ARG
        assert "m_of[%d]" % at in _err()
        assert _host(L, eng, pb, pb, pbad, 3, T, pb, 2, None, pb, pb, pb, pb, 4, pb, pb) == E_ARG and "m_of[%d]" % at in _err()
        assert L.bpp_verify_find_outputs_workspace_bytes(eng, pbad, 3, 2) == 0
    # n_keys x n_out over the bound (n_out = 7): just over it, a factor alone over it, products that wrap 64 bits, and a
    # count that must not be used to read m_of
    for count, nk in ((3, BOUND // 7 + 1), (3, BOUND + 1), (3, 1 << 62), (3, (1 << 64) // 7 + 1), (3, 1 << 63), (3, (1 << 64) - 1),
                      (1 << 63, 2), ((1 << 64) - 1, 1)):
        assert _device(L, eng, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, pb, 4, pb, pb, pb, 1 << 20) == E_ARG
        assert "n_keys x n_out too large" in _err(), (count, nk)
        assert _host(L, eng, pb, pb, pm, count, T, pb, nk, None, pb, pb, pb, pb, 4, pb, pb) == E_ARG
        assert "n_keys x n_out too large" in _err(), (count, nk)
        assert L.bpp_verify_find_outputs_workspace_bytes(eng, pm, count, nk) == 0
    # bound + 1 pairs exactly, by the outputs alone (2^25 under one key) and by the product (2 x 2^24); at 2^24 pairs the
    # pair check passes and the next check answers
    big = np.array([1 << 24, 1 << 24], dtype=np.uint32)
    pbig = big.ctypes.data_as(ctypes.c_void_p)
    assert BOUND + 1 == 1 << 25
    assert _host(L, eng, pb, pb, pbig, 2, T, pb, 1, None, pb, pb, pb, pb, 4, pb, pb) == E_ARG and "n_keys x n_out too large" in _err()
    assert _host(L, eng, pb, pb, pbig, 1, 0, pb, 2, None, pb, pb, pb, pb, 4, pb, pb) == E_ARG and "n_keys x n_out too large" in _err()
    assert _host(L, eng, pb, pb, pbig, 1, 0, pb, 1, None, pb, pb, pb, pb, 4, pb, pb) == E_ARG and "BPP_SER_TRANSCRIPT" in _err()
    # keys that are not word-aligned; a workspace of no bytes (a short one needs the engine: tests/test_gpu_outputs.py)
    odd = ctypes.c_void_p(pb.value + 1)
    assert _device(L, eng, pb, pb, pm, 3, T, odd, 2, None, pb, pb, pb, pb, 4, pb, pb, pb, 1 << 20) == E_ARG and "aligned" in _err()
    assert _device(L, eng, pb, pb, pm, 3, T, pb, 2, None, pb, pb, pb, pb, 4, pb, pb, pb, 0) == E_ARG
    assert "workspace too small" in _err()
    # the host twin with no proof: BPP_OK, no hit and no candidate, whatever else is NULL
    for count, nk in ((0, 2), (0, 0)):
        n = np.full(2, 0x77, dtype=np.uint32)
        assert _host(L, eng, None, None, None, count, T, None, nk, None, None, None, None, None, 0,
                     n[:1].ctypes.data_as(ctypes.c_void_p), n[1:].ctypes.data_as(ctypes.c_void_p)) == 0
        assert n.tolist() == [0, 0]
        n[:] = 0x77
        assert _host(L, eng, None, None, None, count, T, None, nk, None, None, None, None, None, 0,
                     n[:1].ctypes.data_as(ctypes.c_void_p), None) == 0
        assert n.tolist() == [0, 0x77]
    for v, m in ((None, pm), (eng, None)):
        assert L.bpp_verify_find_outputs_workspace_bytes(v, m, 3, 2) == 0
    assert buf.tolist() == [0x77] * 64   # nothing was written


def test_making_outputs_usage_errors():
    L = _lib()
    buf, pb = _bufs()
    # a NULL ctx, each input NULL, all three outputs NULL
    assert L.bpp_outputs_make_device(None, pb, pb, pb, pb, 3, pb, pb, pb, None) == E_ARG and "null" in _err()
    assert L.bpp_outputs_make(None, pb, pb, pb, pb, 3, pb, pb, pb) == E_ARG and "null" in _err()
    for i in range(4):
        a = [pb, pb, pb, pb]
        a[i] = None
        assert L.bpp_outputs_make_device(pb, a[0], a[1], a[2], a[3], 3, pb, pb, pb, None) == E_ARG and "null" in _err(), i
        assert L.bpp_outputs_make(pb, a[0], a[1], a[2], a[3], 3, pb, pb, pb) == E_ARG and "null" in _err(), i
    for n_out in (3, 0):
        assert L.bpp_outputs_make_device(pb, pb, pb, pb, pb, n_out, None, None, None, None) == E_ARG and "null" in _err()
        assert L.bpp_outputs_make(pb, pb, pb, pb, pb, n_out, None, None, None) == E_ARG and "null" in _err()
    odd = ctypes.c_void_p(pb.value + 2)
    assert L.bpp_outputs_make_device(pb, odd, pb, pb, pb, 3, pb, pb, pb, None) == E_ARG and "aligned" in _err()
    for n_out in (BOUND + 1, 1 << 32, 1 << 63):
        assert L.bpp_outputs_make_device(pb, pb, pb, pb, pb, n_out, pb, pb, pb, None) == E_ARG and "too large" in _err()
        assert L.bpp_outputs_make(pb, pb, pb, pb, pb, n_out, pb, None, None) == E_ARG and "too large" in _err()
    # nothing to make of no output: BPP_OK, inputs unread
    assert L.bpp_outputs_make_device(pb, None, None, None, None, 0, pb, None, None, None) == 0
    assert L.bpp_outputs_make(pb, None, None, None, None, 0, None, pb, None) == 0
    assert buf.tolist() == [0x77] * 64
