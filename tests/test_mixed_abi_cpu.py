"""CPU: the mixed-batch entry points (bpp_verifier_run_mixed and friends) are declared, exported and bound, and their
usage errors are return codes, not crashes (no GPU needed: nothing reaches a device)."""

import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = ("bpp_verifier_mixed_workspace_bytes", "bpp_verifier_run_mixed", "bpp_verifier_derive_challenges_mixed",
         "bpp_range_verify_batch_mixed")


def test_mixed_symbols_are_declared_exported_and_bound():
    from bulletproofsplus_amd import _lib
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpp_amd.h")).read(), flags=re.S)
    for s in MIXED:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.EXPORTS, s
        assert hasattr(L, s), s
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for s in MIXED:
        assert "pub fn %s(" % s in ffi, s


def test_mixed_null_arguments_are_errors():
    from bulletproofsplus_amd import _lib
    L = _lib.lib()
    ms = np.array([1, 2, 4], dtype=np.uint32)
    pm = ms.ctypes.data_as(ctypes.c_void_p)
    buf = np.zeros(64, dtype=np.uint64)
    pb = buf.ctypes.data_as(ctypes.c_void_p)
    # a null verifier: 0 bytes, and a usage error from every call, whatever the other arguments
    assert L.bpp_verifier_mixed_workspace_bytes(None, pm, 3) == 0
    assert L.bpp_verifier_mixed_workspace_bytes(None, None, 0) == 0
    assert L.bpp_verifier_run_mixed(None, pb, pb, pm, 3, None, pb, pb, 1 << 20, None, None) < 0
    assert L.bpp_verifier_run_mixed(None, None, None, None, 3, None, None, None, 0, None, None) < 0
    assert L.bpp_verifier_run_mixed(None, None, None, None, 0, None, None, None, 0, None, None) < 0
    assert L.bpp_verifier_derive_challenges_mixed(None, pb, pm, 3, pb, pb, 1 << 20, None) < 0
    assert L.bpp_verifier_derive_challenges_mixed(None, None, None, 3, None, None, 0, None) < 0
    assert L.bpp_range_verify_batch_mixed(None, pb, pb, pm, 3, pb) < 0
    assert L.bpp_range_verify_batch_mixed(None, None, None, None, 3, None) < 0
    assert "null" in L.bpp_last_error().decode()
