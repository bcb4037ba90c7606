"""CPU: the cut of a batch over the shards of a verifier pool and the thread fan-out (csrc/shard.hpp; include/bpp_amd.h
"verifier pool").

 * tests/host/shard_host_test.cpp, a stand-alone host build (g++; under ASan + UBSan with BPP_HOST_SANITIZE=1, and once
   under the thread sanitizer): the worked cut vectors, the uniform rule against its formula, monotony / cover / balance
   on seeded random costs, the argument errors, and run_shards' error slots and joins.
 * bpp_shard_cuts through the library equals sharding.shard_bounds, and api.shard_cuts gives the worked vectors."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_host_arith_cpu import SANITIZE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "shard_host_test.cpp")


def _build(tmp_path, tag, flags):
    exe = str(tmp_path / ("bpp_shard_host_test_" + tag))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread"] + flags + ["-o", exe, SRC])
    return exe


def test_cuts_and_fan_out_host_build(tmp_path):
    out = subprocess.run([_build(tmp_path, "san" if SANITIZE else "plain", SANITIZE)], capture_output=True, text=True)
    assert out.returncode == 0 and "ok shard" in out.stdout, out.stdout + out.stderr


def test_fan_out_under_the_thread_sanitizer(tmp_path):
    out = subprocess.run([_build(tmp_path, "tsan", ["-fsanitize=thread", "-g"])], capture_output=True, text=True)
    assert out.returncode == 0 and "ok shard" in out.stdout and "ThreadSanitizer" not in out.stderr, out.stdout + out.stderr


def _lib():
    from bulletproofsplus_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_uniform_cut_equals_shard_bounds():
    from bulletproofsplus_amd import sharding
    L = _lib()
    for count in range(0, 51):
        for world in range(1, 10):
            cuts = (ctypes.c_size_t * (world + 1))()
            assert L.bpp_shard_cuts(None, count, world, cuts) == 0
            bounds = [sharding.shard_bounds(count, world, r) for r in range(world)]
            assert list(cuts) == [lo for lo, _ in bounds] + [count]
            assert all(cuts[r + 1] == hi for r, (_, hi) in enumerate(bounds))


@pytest.mark.parametrize("ms, count, world, want", [
    (None, 10, 4, [0, 3, 6, 8, 10]),
    (None, 2, 3, [0, 1, 2, 2]),
    ([16, 1, 1, 1, 1, 1, 1, 1, 1, 8], 10, 2, [0, 1, 10]),
    ([1, 1, 16, 1, 1], 5, 3, [0, 3, 3, 5]),
])
def test_python_shard_cuts_worked_values(ms, count, world, want):
    import bulletproofsplus_amd as B
    _lib()
    assert B.shard_cuts(ms, count, world).tolist() == want


def test_shard_cuts_errors():
    import bulletproofsplus_amd as B
    L = _lib()
    cuts = (ctypes.c_size_t * 18)()
    for world in (0, 17):
        assert L.bpp_shard_cuts(None, 4, world, cuts) == -1
    assert L.bpp_shard_cuts(None, 4, 2, None) == -1
    assert L.bpp_shard_cuts(None, 1 << 32, 2, cuts) == -1
    m = np.array([1, 2, 0, 4], dtype=np.uint32)
    assert L.bpp_shard_cuts(m.ctypes.data_as(ctypes.c_void_p), 4, 2, cuts) == -1
    assert b"m_of[2]" in L.bpp_last_error()
    with pytest.raises(B.BppError):
        B.shard_cuts([1, 0], 2, 2)
