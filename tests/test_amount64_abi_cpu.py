"""CPU: BPP_PROVE_AMOUNT64 and the batched commitment entries (bpp_commit_batch_device, bpp_commit_batch) are declared,
exported, bound and present in the Rust FFI; the commit entries run under a guard shim; usage errors are return codes that
leave the caller's buffers alone; the four mixed prove calls know the flag.  No GPU needed: nothing here reaches a device
(an argument check answers before the engine handle is read, so a dummy non-null handle stands in for one)."""

import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bpp_commit_batch_device", "bpp_commit_batch")
AMOUNT64 = 0x100


def _lib():
    from bulletproofsplus_amd import _lib as M
    return M.lib()


def test_flag_and_entries_are_declared_exported_and_bound():
    from bulletproofsplus_amd import _lib as M
    from bulletproofsplus_amd import api
    L = M.lib()
    raw = open(os.path.join(ROOT, "include", "bpp_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    m = re.search(r"^#define\s+BPP_PROVE_AMOUNT64\s+(\S+)\s*$", hdr, flags=re.M)
    assert m and int(m.group(1), 0) == 0x100 == api.AMOUNT64
    assert re.search(r"pub const BPP_PROVE_AMOUNT64: \w+ = (0x100|256);", ffi)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in M.EXPORTS, s
        assert hasattr(L, s), s
        assert "pub fn %s(" % s in ffi, s
    # the comment in front of the new entries, and the flag's on the mixed prove calls, cite the truncation they lift
    block = raw[raw.index("commitments for a block of amounts"):raw.index("int bpp_commit_batch(")]
    assert "src/range/prover.rs:28-42" in block and "src/range/prover.rs:37" in block
    block = raw[raw.index("PROVING blocks of mixed aggregation sizes"):raw.index("bpp_range_prove_batch_serialized_mixed(")]
    assert block.count("src/range/prover.rs:37") >= 3 and "BPP_PROVE_AMOUNT64" in block


def test_commit_entries_run_under_the_guard():
    import test_abi_guard_cpu as G
    entries = G._entry_points(open(os.path.join(ROOT, "bulletproofsplus_amd", "csrc", "capi.hip")).read())
    for s in SYMBOLS:
        assert s in entries and any(shim in entries[s] for shim in G.SHIMS), s
        assert '{count, "count"}' in entries[s], (s, "count is not bounded by the shim")


def _bufs():
    buf = np.full(64, 0x77, dtype=np.uint64)
    return buf, buf.ctypes.data_as(ctypes.c_void_p)


def test_commit_usage_errors_leave_the_buffers_alone():
    L = _lib()
    buf, pb = _bufs()
    eng = pb   # never read: every case below is answered by an argument check
    for f, tail in ((L.bpp_commit_batch_device, (None,)), (L.bpp_commit_batch, ())):
        assert f(None, pb, pb, 3, 0, pb, *tail) < 0 and "null" in L.bpp_last_error().decode()
        assert f(None, pb, pb, 0, 0, pb, *tail) < 0                       # a NULL engine even with nothing to do
        for args in ((None, pb, pb), (pb, None, pb), (pb, pb, None)):
            for flags in (0, AMOUNT64):
                assert f(eng, args[0], args[1], 3, flags, args[2], *tail) < 0
                assert "null" in L.bpp_last_error().decode()
        for flags in (AMOUNT64 | 4, 1, 2, 4, AMOUNT64 | 1, 0x200, -1):
            assert f(eng, pb, pb, 3, flags, pb, *tail) < 0
            assert "unknown flag" in L.bpp_last_error().decode(), flags
        assert f(eng, pb, pb, 0, AMOUNT64 | 4, pb, *tail) < 0             # ... also with count = 0
        assert f(eng, None, None, 0, 0, None, *tail) == 0                 # count = 0 is BPP_OK
        assert f(eng, None, None, 0, AMOUNT64, None, *tail) == 0
    assert buf.tolist() == [0x77] * 64   # nothing was written


def test_mixed_prove_calls_know_the_flag():
    """flags = BPP_PROVE_AMOUNT64 (alone, or with the flags each call already takes) passes the flag check: with NULL
    buffers the answer is the NULL-pointer text, not "unknown flag".  Bits 2 / 4 stay unknown where they were."""
    L = _lib()
    buf, pb = _bufs()
    eng = pb
    ms = np.array([1, 2, 1], dtype=np.uint32)
    pm = ms.ctypes.data_as(ctypes.c_void_p)
    calls = (
        (lambda fl: L.bpp_range_prove_batch_mixed_device(eng, None, None, pm, 3, fl, None, 0, None, None, None, None, None, 0, None),
         (AMOUNT64, AMOUNT64 | 1), (AMOUNT64 | 2, AMOUNT64 | 4, 0x200)),
        (lambda fl: L.bpp_range_prove_batch_serialized_mixed_device(eng, None, None, pm, 3, fl, None, 0, None, None, None, None, 0, None),
         (AMOUNT64, AMOUNT64 | 1, AMOUNT64 | 2, AMOUNT64 | 3), (AMOUNT64 | 4, 0x200)),
        (lambda fl: L.bpp_range_prove_batch_mixed(eng, None, None, pm, 3, fl, None, 0, None, None, None),
         (AMOUNT64, AMOUNT64 | 1), (AMOUNT64 | 2, AMOUNT64 | 4, 0x200)),
        (lambda fl: L.bpp_range_prove_batch_serialized_mixed(eng, None, None, pm, 3, fl, None, 0, None, None),
         (AMOUNT64, AMOUNT64 | 1, AMOUNT64 | 2, AMOUNT64 | 3), (AMOUNT64 | 4, 0x200)),
    )
    for call, known, unknown in calls:
        for fl in known:
            assert call(fl) < 0
            assert "null" in L.bpp_last_error().decode() and "unknown flag" not in L.bpp_last_error().decode(), hex(fl)
        for fl in unknown:
            assert call(fl) < 0
            assert "unknown flag" in L.bpp_last_error().decode(), hex(fl)
    assert buf.tolist() == [0x77] * 64


def test_other_entries_do_not_know_the_flag():
    L = _lib()
    buf, pb = _bufs()
    assert L.bpp_wip_prove_batch_device(pb, pb, pb, pb, pb, 1, 1, AMOUNT64, None, None, 0, None, pb, pb, None, pb, 1 << 20, None) < 0
    assert "unknown flag" in L.bpp_last_error().decode()
    assert buf.tolist() == [0x77] * 64


def test_wrappers_exist():
    import inspect
    import bulletproofsplus_amd as B
    for name in ("commit_batch", "commit_batch_device"):
        assert callable(getattr(B.BatchVerifier, name)), name
    for name in ("prove_mixed_device", "prove_serialized_mixed_device", "prove_batch_mixed", "prove_serialized_mixed",
                 "prove_batch", "commit_batch", "commit_batch_device"):
        assert inspect.signature(getattr(B.BatchVerifier, name)).parameters["amount64"].default is False, name
    assert inspect.signature(B.RangeProver.commit).parameters["amount64"].default is False
