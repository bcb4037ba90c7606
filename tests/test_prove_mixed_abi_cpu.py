"""CPU: the entry points that PROVE blocks of mixed aggregation sizes (bpp_range_prove_batch_mixed_device and friends) are
declared, exported, bound and present in the Rust FFI; each cites its reference site in the header; their usage errors are
return codes, not crashes.  No GPU needed: nothing here reaches a device."""

import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bpp_prover_mixed_workspace_bytes", "bpp_range_prove_batch_mixed_device",
           "bpp_prover_serialized_mixed_workspace_bytes", "bpp_range_prove_batch_serialized_mixed_device",
           "bpp_range_prove_batch_mixed", "bpp_range_prove_batch_serialized_mixed")


def _lib():
    from bulletproofsplus_amd import _lib as M
    return M.lib()


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
    # every new entry cites its reference site: the comment block in front of the first of them names the reference's files
    block = raw[raw.index("PROVING blocks of mixed aggregation sizes"):raw.index("bpp_range_prove_batch_serialized_mixed(")]
    for site in ("src/range/mod.rs:31-55", ":80-187", ":240-403", "src/weighted_inner_product_proof.rs:36-227",
                 "src/range/prover.rs:28-42"):
        assert site in block, site


def test_entries_run_under_the_guard():
    import test_abi_guard_cpu as G
    entries = G._entry_points(open(os.path.join(ROOT, "bulletproofsplus_amd", "csrc", "capi.hip")).read())
    for s in SYMBOLS:
        assert s in entries and any(shim in entries[s] for shim in G.SHIMS), s


def test_null_arguments_are_errors():
    L = _lib()
    ms = np.array([1, 2, 4], dtype=np.uint32)
    pm = ms.ctypes.data_as(ctypes.c_void_p)
    buf = np.full(64, 0x77, dtype=np.uint64)
    pb = buf.ctypes.data_as(ctypes.c_void_p)
    key = bytes(32)
    for f in (L.bpp_prover_mixed_workspace_bytes, L.bpp_prover_serialized_mixed_workspace_bytes):
        assert f(None, pm, 3) == 0
        assert f(None, None, 0) == 0
        assert f(None, None, 3) == 0
    assert L.bpp_range_prove_batch_mixed_device(None, pb, pb, pm, 3, 0, None, 0, None, pb, pb, pb, pb, 1 << 20, None) < 0
    assert "null" in L.bpp_last_error().decode()
    assert L.bpp_range_prove_batch_mixed_device(None, None, None, None, 0, 0, None, 0, None, None, None, None, None, 0, None) < 0
    assert L.bpp_range_prove_batch_mixed_device(None, pb, pb, pm, 3, 1, key, 5, pb, pb, pb, None, pb, 1 << 20, None) < 0
    assert L.bpp_range_prove_batch_serialized_mixed_device(None, pb, pb, pm, 3, 3, None, 0, None, pb, pb, pb, 1 << 20, None) < 0
    assert "null" in L.bpp_last_error().decode()
    assert L.bpp_range_prove_batch_serialized_mixed_device(None, None, None, None, 0, 0, None, 0, None, None, None, None, 0, None) < 0
    assert L.bpp_range_prove_batch_mixed(None, pb, pb, pm, 3, 0, None, 0, pb, pb, None) < 0
    assert "null" in L.bpp_last_error().decode()
    assert L.bpp_range_prove_batch_mixed(None, None, None, None, 3, 1, key, 0, None, None, None) < 0
    assert L.bpp_range_prove_batch_serialized_mixed(None, pb, pb, pm, 3, 0, None, 0, pb, pb) < 0
    assert "null" in L.bpp_last_error().decode()
    assert L.bpp_range_prove_batch_serialized_mixed(None, None, None, None, 0, 2, None, 0, None, None) < 0
    assert buf.tolist() == [0x77] * 64   # nothing was written


def test_wrappers_exist():
    import bulletproofsplus_amd as B
    for name in ("prover_mixed_workspace_bytes", "prove_mixed_device", "prove_serialized_mixed_device", "prove_batch_mixed",
                 "prove_serialized_mixed"):
        assert callable(getattr(B.BatchVerifier, name)), name
