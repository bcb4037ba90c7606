"""CPU: the verifier pool's C ABI without a device (include/bpp_amd.h "verifier pool"; csrc/pool.hpp).

The nine symbols are declared, exported, bound and mirrored in the Rust ffi block, their entries run under the shims, the
argument errors come back as BPP_E_ARG before anything is touched, and bpp_pool_create on a machine without a GPU fails
with BPP_E_HIP, leaves *out NULL and the process alive."""

import ctypes
import os
import sys

import numpy as np

from test_abi_guard_cpu import SHIMS, _entry_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rust_ffi as G  # noqa: E402

POOL = ("bpp_shard_cuts", "bpp_pool_create", "bpp_pool_destroy", "bpp_pool_size", "bpp_pool_device", "bpp_pool_verifier",
        "bpp_pool_verify_mixed", "bpp_pool_verify_serialized_mixed", "bpp_pool_verify_combined")
E_ARG, E_HIP = -1, -2


def _load():
    from bulletproofsplus_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def _err(L):
    return L.bpp_last_error().decode()


def test_pool_symbols_in_every_layer():
    from bulletproofsplus_amd import _lib
    L = _load()
    header = open(os.path.join(ROOT, "include", "bpp_amd.h")).read()
    declared = {n for n, _, _ in G.c_prototypes(header)}
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    entries = _entry_points(open(os.path.join(ROOT, "bulletproofsplus_amd", "csrc", "capi.hip")).read())
    for name in POOL:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
        assert "pub fn %s(" % name in ffi, name
        assert name in entries and any(s in entries[name] for s in SHIMS), name
    assert "BPP_POOL_EXACT 0" in header and "BPP_POOL_GROUPED 1" in header
    assert "pub const BPP_POOL_GROUPED: c_int = 1;" in ffi
    # the block names the reference fact it rests on: each proof ends in its own check
    block = header[header.index("verifier pool: ONE batch"):header.index("#define BPP_POOL_EXACT")]
    assert "src/range/mod.rs:503-509" in block
    assert "DEPEND ON THE CUT" in block and "only for bpp_pool_destroy" in block


def _key_args():
    """(gh, G, H) buffers of the right size for BLS12-381 (8, 4); the values never reach a device in this file"""
    pw = 13
    return (np.zeros((2, pw), np.uint64), np.zeros((32, pw), np.uint64), np.zeros((32, pw), np.uint64))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_pool_create_argument_errors():
    L = _load()
    gh, Gv, Hv = _key_args()
    dev = np.zeros(17, dtype=np.int32)
    for n_dev in (0, 17):
        out = ctypes.c_void_p(0xdead)
        assert L.bpp_pool_create(0, _p(dev), n_dev, _p(gh), _p(Gv), _p(Hv), 8, 4, 5, ctypes.byref(out)) == E_ARG
        assert not out.value and "n_dev" in _err(L)
    for null_at in (1, 3, 4, 5):
        out = ctypes.c_void_p(0xdead)
        argv = [0, _p(dev), 1, _p(gh), _p(Gv), _p(Hv), 8, 4, 5, ctypes.byref(out)]
        argv[null_at] = None
        assert L.bpp_pool_create(*argv) == E_ARG, null_at
        assert not out.value and "null" in _err(L)
    assert L.bpp_pool_create(0, _p(dev), 1, _p(gh), _p(Gv), _p(Hv), 8, 4, 5, None) == E_ARG


def test_pool_create_without_a_usable_device_fails_cleanly():
    """valid arguments, but ordinals no machine has: without a GPU the device count itself fails, with one the ordinal is
    refused -- BPP_E_HIP either way, from the lowest shard, nothing built is left behind and the process survives"""
    L = _load()
    gh, Gv, Hv = _key_args()
    for devices in ([1000000], [1000000, 1000001, 1000000]):
        dev = np.array(devices, dtype=np.int32)
        out = ctypes.c_void_p(0xdead)
        rc = L.bpp_pool_create(0, _p(dev), len(dev), _p(gh), _p(Gv), _p(Hv), 8, 4, 5, ctypes.byref(out))
        assert rc == E_HIP and not out.value, (rc, out.value)
        assert _err(L).startswith("shard 0 (device 1000000): "), _err(L)
    assert L.bpp_pool_size(None) == 0   # the process is alive and the library answers


def test_null_pool():
    L = _load()
    assert L.bpp_pool_size(None) == 0
    assert L.bpp_pool_device(None, 0) == -1
    v = ctypes.c_void_p(0xdead)
    assert L.bpp_pool_verifier(None, 0, ctypes.byref(v)) == E_ARG and not v.value and "null" in _err(L)
    assert L.bpp_pool_verifier(None, 0, None) == E_ARG
    L.bpp_pool_destroy(None)
    ok = np.full(4, 7, dtype=np.uint32)
    stats = np.full(2, 9, dtype=np.uint64)
    buf = np.zeros(4096, dtype=np.uint64)
    m = np.array([1, 2, 4, 1], dtype=np.uint32)
    key = bytes(32)
    assert L.bpp_pool_verify_mixed(None, _p(buf), _p(buf), _p(m), 4, _p(ok)) == E_ARG and "null" in _err(L)
    for mode in (0, 1):
        assert L.bpp_pool_verify_serialized_mixed(None, _p(buf), _p(buf), _p(m), 4, 0, mode, key, 0, 4, _p(ok), _p(stats)) == E_ARG
        assert "null" in _err(L)
    assert L.bpp_pool_verify_combined(None, _p(buf), _p(buf), 4, key, 0, _p(ok)) == E_ARG and "null" in _err(L)
    assert ok.tolist() == [7] * 4 and stats.tolist() == [9, 9]
