"""CPU: the grouped check over mixed batches (bpp_verifier_run_grouped_mixed and friends) is declared, exported and bound,
its usage errors are return codes, and mixed_groups -- the documented partition callers predict `stats` from -- follows
the rule the header states (no GPU needed: nothing reaches a device)."""

import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPED_MIXED = ("bpp_verifier_grouped_mixed_workspace_bytes", "bpp_verifier_run_grouped_mixed",
                 "bpp_verifier_serialized_grouped_mixed_workspace_bytes",
                 "bpp_range_verify_batch_serialized_grouped_mixed_device")


def test_grouped_mixed_symbols_are_declared_exported_and_bound():
    from bulletproofsplus_amd import _lib
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpp_amd.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for s in GROUPED_MIXED:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.EXPORTS, s
        assert hasattr(L, s), s
        assert "pub fn %s(" % s in ffi, s


def test_grouped_mixed_null_arguments_are_errors():
    from bulletproofsplus_amd import _lib
    L = _lib.lib()
    ms = np.array([1, 2, 4], dtype=np.uint32)
    pm = ms.ctypes.data_as(ctypes.c_void_p)
    buf = np.zeros(64, dtype=np.uint64)
    pb = buf.ctypes.data_as(ctypes.c_void_p)
    key = bytes(32)
    # a null verifier: 0 bytes, and a usage error from every call, whatever the other arguments
    for f in (L.bpp_verifier_grouped_mixed_workspace_bytes, L.bpp_verifier_serialized_grouped_mixed_workspace_bytes):
        assert f(None, pm, 3, 4) == 0
        assert f(None, None, 0, 4) == 0
    for count in (3, 0):
        assert L.bpp_verifier_run_grouped_mixed(None, pb, pb, pm, count, None, key, 0, None, 4, pb, pb, pb, 1 << 20, None) < 0
        assert "null" in L.bpp_last_error().decode()
        assert L.bpp_verifier_run_grouped_mixed(None, None, None, None, count, None, None, 0, None, 4, None, None, None, 0,
                                                None) < 0
        assert L.bpp_range_verify_batch_serialized_grouped_mixed_device(None, pb, pb, pm, count, 0, key, 0, 4, pb, pb, pb,
                                                                        1 << 20, None) < 0
        assert "null" in L.bpp_last_error().decode()
        assert L.bpp_range_verify_batch_serialized_grouped_mixed_device(None, None, None, None, count, 0, None, 0, 4, None,
                                                                        None, None, 0, None) < 0
    assert "null" in L.bpp_last_error().decode()


def _groups_by_the_rule(ms, group):
    """the header's rule, restated: gather the classes ascending, caller order within a class; cut runs of `group`"""
    gathered = []
    for c in sorted(set(ms)):
        gathered += [i for i, m in enumerate(ms) if m == c]
    out = [None] * len(ms)
    for pos, i in enumerate(gathered):
        out[i] = pos // group
    return out


def test_mixed_groups_is_the_documented_partition():
    from bulletproofsplus_amd import mixed_groups
    rng = np.random.default_rng(11)
    for trial in range(200):
        count = int(rng.integers(0, 70))
        classes = [1, 2, 4, 8, 16][:int(rng.integers(1, 6))]
        if trial % 3 == 0 and len(classes) > 2:
            classes = classes[::2]                         # empty classes in between
        ms = [int(x) for x in rng.choice(classes, size=count)]
        for group in (2, 4, 8, 32, 128):
            got = mixed_groups(ms, group)
            assert got.tolist() == _groups_by_the_rule(ms, group), (ms, group)
            assert len(got) == count
    # the example of the issue: 3, 5, 2 proofs of m = 1, 2, 4 at group 4, callers shuffled
    ms = [2, 1, 4, 2, 2, 1, 2, 4, 1, 2]
    g = mixed_groups(ms, 4).tolist()
    assert g == _groups_by_the_rule(ms, 4)
    assert sorted(g) == [0] * 4 + [1] * 4 + [2] * 2                       # a ragged last group
    assert [ms[i] for i in range(10) if g[i] == 0].count(1) == 3          # group 0: three m = 1 proofs and one m = 2
    assert mixed_groups([4] * 7, 4).tolist() == [0, 0, 0, 0, 1, 1, 1]     # a single class
    assert mixed_groups([1, 16, 1, 16], 2).tolist() == [0, 1, 0, 1]       # empty classes in between
    assert mixed_groups([2, 1, 2], 32).tolist() == [0, 0, 0]              # group larger than the batch
    assert mixed_groups([], 4).tolist() == []
    for bad in (0, 1, 3, 12):
        with pytest.raises(ValueError):
            mixed_groups([1, 2], bad)
