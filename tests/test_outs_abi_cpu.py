"""CPU: the calls for proofs over any number of outputs (bpp_outs_shapes, the *_outs* prove, verify, grouped and find
entries and their workspace getters) are declared, exported, bound and present in the Rust FFI; they run under the entry
shim; the wrappers exist; the rule gives [1, 2, 4, 4, 8, 8, 8, 8] for 1..8 and names the index it refuses; null arguments
and count = 0 are codes, not crashes; the size getters answer 0 for what is not taken.  And csrc/outs_plan.hpp in a host
build (tests/host/outs_plan_host_test.cpp; ASan + UBSan with BPP_HOST_SANITIZE=1) against a plain recomputation.
No GPU needed: every case here is answered before the engine handle is read, so a dummy non-null handle stands in for
one.  The cases that need the engine are in tests/test_gpu_outs.py."""

import ctypes
import os
import re
import subprocess

import numpy as np

from test_host_arith_cpu import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ("bpp_prover_serialized_outs_workspace_bytes", "bpp_verifier_serialized_outs_workspace_bytes",
         "bpp_verifier_serialized_grouped_outs_workspace_bytes", "bpp_verify_find_outputs_outs_workspace_bytes")
CALLS = ("bpp_range_prove_batch_serialized_outs_device", "bpp_range_prove_batch_serialized_outs",
         "bpp_range_verify_batch_serialized_outs_device", "bpp_range_verify_batch_serialized_outs",
         "bpp_range_verify_batch_serialized_grouped_outs_device",
         "bpp_range_verify_find_outputs_serialized_outs_keys_device", "bpp_range_verify_find_outputs_serialized_outs_keys")
ALL = ("bpp_outs_shapes",) + SIZES + CALLS
TRANSCRIPT = 1
E_ARG = -1


def _lib():
    from bulletproofsplus_amd import _lib as M
    return M.lib()


def _err():
    return _lib().bpp_last_error().decode()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_are_declared_exported_and_bound():
    from bulletproofsplus_amd import _lib as M
    L = M.lib()
    raw = open(os.path.join(ROOT, "include", "bpp_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for s in ALL:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in M.EXPORTS, s
        assert hasattr(L, s), s
        assert "pub fn %s(" % s in ffi, s
    block = re.sub(r"[\s*]+", " ", raw[raw.index("proofs over ANY number of outputs"):raw.index("the weighted inner product argument")])
    for text in ("M = 2^ceil(log2 o)", "are the identity", "THE OUTPUT COUNT IS NOT AUTHENTICATED", "are the same statement",
                 "binds the transaction's output list outside the proof", "bpp_proofs_scan returns M",
                 "need no ragged form: they are per output"):
        assert text in block, text


def test_entries_run_under_the_guard():
    import test_abi_guard_cpu as G
    entries = G._entry_points(open(os.path.join(ROOT, "bulletproofsplus_amd", "csrc", "capi.hip")).read())
    for s in ALL:
        assert s in entries and any(shim in entries[s] for shim in G.SHIMS), s
    for s in CALLS:
        # one argument record per family, the checks of the mixed entries
        assert re.search(r"\b(VerifyArgs|ProveArgs|FindArgs) a\b", entries[s]), s
        assert "a.outs_of = outs_of" in entries[s], s
        assert re.search(r"\b(verify_args|prove_args|find_args)\(", entries[s]), s


def test_wrappers_exist():
    import inspect

    import bulletproofsplus_amd as B
    from bulletproofsplus_amd import api
    for name in ("prove_serialized_outputs", "prove_serialized_outputs_device", "verify_serialized_outputs",
                 "verify_serialized_outputs_device", "verify_find_outputs_serialized_outs_keys",
                 "verify_find_outputs_serialized_outs_keys_device"):
        assert callable(getattr(B.BatchVerifier, name)), name
    sig = inspect.signature(B.BatchVerifier.verify_serialized_outputs).parameters
    assert list(sig)[1:] == ["proofs", "commitments", "outs", "transcript", "uncompressed", "group"]
    assert sig["group"].default is None
    assert callable(api.outs_shapes) and B.outs_shapes is api.outs_shapes
    hpp = open(os.path.join(ROOT, "include", "bpp_amd.hpp")).read()
    for s in ("bpp_outs_shapes(", "bpp_range_prove_batch_serialized_outs(", "bpp_range_verify_batch_serialized_outs(",
              "bpp_range_verify_find_outputs_serialized_outs_keys("):
        assert s in hpp, s
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for s in ("pub fn outs_shapes(", "pub fn prove_serialized_outputs(", "pub fn verify_serialized_outputs(",
              "pub fn verify_find_outputs_serialized_outs_keys(", "ffi::bpp_outs_shapes(",
              "ffi::bpp_range_prove_batch_serialized_outs(", "ffi::bpp_range_verify_batch_serialized_outs(",
              "ffi::bpp_range_verify_find_outputs_serialized_outs_keys("):
        assert s in rs, s
    # the Rust wrappers check their lengths before the FFI call
    for fn in ("verify_serialized_outputs", "verify_find_outputs_serialized_outs_keys"):
        body = rs[rs.index("pub fn %s(" % fn):]
        assert body.index("return Err(ProofError::FormatError)") < body.index("ffi::bpp_range_"), fn


def test_the_rule():
    from bulletproofsplus_amd import api
    from bulletproofsplus_amd._lib import BppError
    assert api.outs_shapes(list(range(1, 9)), 8).tolist() == [1, 2, 4, 4, 8, 8, 8, 8]
    assert api.outs_shapes([], 8).tolist() == []
    assert api.outs_shapes([128, 65, 64, 33], 128).tolist() == [128, 128, 64, 64]
    L = _lib()
    for cap in (1, 4, 8, 16):
        for at in range(3):
            for bad in (0, cap + 1):
                outs = np.ones(3, dtype=np.uint32)
                outs[at] = bad
                ms = np.full(3, 0x77, dtype=np.uint32)
                assert L.bpp_outs_shapes(_p(outs), 3, cap, _p(ms)) == E_ARG
                assert "outs_of[%d] = %d" % (at, bad) in _err()
                try:
                    api.outs_shapes(outs, cap)
                    assert False
                except BppError as e:
                    assert e.code == E_ARG and "outs_of[%d]" % at in str(e)
    # null arguments and no work
    one = np.ones(1, dtype=np.uint32)
    assert L.bpp_outs_shapes(None, 0, 8, None) == 0
    assert L.bpp_outs_shapes(None, 1, 8, _p(one)) == E_ARG and "null" in _err()
    assert L.bpp_outs_shapes(_p(one), 1, 8, None) == E_ARG and "null" in _err()
    assert L.bpp_outs_shapes(_p(one), 1 << 32, 8, _p(one)) == E_ARG and "too large" in _err()


def test_null_arguments_and_empty_blocks_are_codes():
    L = _lib()
    buf = np.full(64, 0x77, dtype=np.uint64)
    pb = _p(buf)
    eng = pb   # never read
    outs = np.array([3, 1, 5], dtype=np.uint32)
    po = _p(outs)
    T, KEY = TRANSCRIPT, bytes(32)
    prove_d = lambda e, v, g, o, c, fl, pr, cm, ws: L.bpp_range_prove_batch_serialized_outs_device(
        e, v, g, o, c, fl, None, 0, None, pr, cm, ws, 1 << 20, None)
    prove_h = lambda e, v, g, o, c, fl, pr, cm: L.bpp_range_prove_batch_serialized_outs(e, v, g, o, c, fl, None, 0, pr, cm)
    ver_d = lambda e, pr, cm, o, c, fl, ok, ws: L.bpp_range_verify_batch_serialized_outs_device(e, pr, cm, o, c, fl, ok, ws, 1 << 20, None)
    ver_h = lambda e, pr, cm, o, c, fl, ok: L.bpp_range_verify_batch_serialized_outs(e, pr, cm, o, c, fl, ok)
    grp_d = lambda e, pr, cm, o, c, fl, key, ok, ws: L.bpp_range_verify_batch_serialized_grouped_outs_device(
        e, pr, cm, o, c, fl, key, 0, 4, ok, None, ws, 1 << 20, None)
    find_d = lambda e, pr, cm, o, c, fl, k, nk, se, tg, ok, h, nh, ws: L.bpp_range_verify_find_outputs_serialized_outs_keys_device(
        e, pr, cm, o, c, fl, k, nk, 5, None, se, tg, ok, h, 4, nh, None, ws, 1 << 20, None)
    find_h = lambda e, pr, cm, o, c, fl, k, nk, se, tg, ok, h, nh: L.bpp_range_verify_find_outputs_serialized_outs_keys(
        e, pr, cm, o, c, fl, k, nk, 5, None, se, tg, ok, h, 4, nh, None)
    # a NULL engine
    assert prove_d(None, pb, pb, po, 3, 0, pb, pb, pb) == E_ARG and "null" in _err()
    assert prove_h(None, pb, pb, po, 3, 0, pb, pb) == E_ARG and "null" in _err()
    assert ver_d(None, pb, pb, po, 3, 0, pb, pb) == E_ARG and "null" in _err()
    assert ver_h(None, pb, pb, po, 3, 0, pb) == E_ARG and "null" in _err()
    assert grp_d(None, pb, pb, po, 3, 0, KEY, pb, pb) == E_ARG and "null" in _err()
    assert find_d(None, pb, pb, po, 3, T, pb, 2, pb, pb, pb, pb, pb, pb) == E_ARG and "null" in _err()
    assert find_h(None, pb, pb, po, 3, T, pb, 2, pb, pb, pb, pb, pb) == E_ARG and "null" in _err()
    # each required pointer, outs_of among them
    for i in range(6):
        a = [pb, pb, po, pb, pb, pb]
        a[i] = None
        assert prove_d(eng, a[0], a[1], a[2], 3, 0, a[3], a[4], a[5]) == E_ARG and "null" in _err(), i
    for i in range(5):
        a = [pb, pb, po, pb, pb]
        a[i] = None
        assert prove_h(eng, a[0], a[1], a[2], 3, 0, a[3], a[4]) == E_ARG and "null" in _err(), i
        assert ver_d(eng, a[0], a[1], a[2], 3, 0, a[3], a[4]) == E_ARG and "null" in _err(), i
    for i in range(4):
        a = [pb, pb, po, pb]
        a[i] = None
        assert ver_h(eng, a[0], a[1], a[2], 3, 0, a[3]) == E_ARG and "null" in _err(), i
    for i in range(6):
        a = [pb, pb, po, KEY, pb, pb]   # proofs, commitments, outs_of, weight_key, ok, ws
        a[i] = None
        assert grp_d(eng, a[0], a[1], a[2], 3, 0, a[3], a[4], a[5]) == E_ARG and "null" in _err(), i
    for i in range(10):
        a = [pb, pb, po, pb, pb, pb, pb, pb, pb, pb]   # proofs, commitments, outs_of, keys, sealed, tags, ok, hits, n_hits, ws
        a[i] = None
        assert find_d(eng, a[0], a[1], a[2], 3, T, a[3], 2, a[4], a[5], a[6], a[7], a[8], a[9]) == E_ARG and "null" in _err(), i
    for i in range(9):
        a = [pb, pb, po, pb, pb, pb, pb, pb, pb]
        a[i] = None
        assert find_h(eng, a[0], a[1], a[2], 3, T, a[3], 2, a[4], a[5], a[6], a[7], a[8]) == E_ARG and "null" in _err(), i
    # unknown flags; the find calls need the transcript
    assert prove_d(eng, pb, pb, po, 3, 4, pb, pb, pb) == E_ARG and "unknown flag" in _err()
    assert ver_d(eng, pb, pb, po, 3, 0x100, pb, pb) == E_ARG and "unknown flag" in _err()
    assert find_d(eng, pb, pb, po, 3, 0, pb, 2, pb, pb, pb, pb, pb, pb) == E_ARG and "BPP_SER_TRANSCRIPT" in _err()
    assert find_h(eng, pb, pb, po, 3, 0, pb, 2, pb, pb, pb, pb, pb) == E_ARG and "BPP_SER_TRANSCRIPT" in _err()
    assert find_d(eng, pb, pb, po, 3, T | 0x200, pb, 2, pb, pb, pb, pb, pb, pb) == E_ARG and "BPP_FIND_AMOUNTS_SEALED" in _err()
    # n_keys x sum(outs) over the bound (9 outputs)
    bound = 0x7fffffff // 64
    for nk in (bound // 9 + 1, bound + 1, 1 << 62, (1 << 64) - 1):
        assert find_h(eng, pb, pb, po, 3, T, pb, nk, pb, pb, pb, pb, pb) == E_ARG and "n_keys x n_out too large" in _err()
        assert L.bpp_verify_find_outputs_outs_workspace_bytes(eng, po, 3, nk) == 0
    # count = 0: BPP_OK with everything else NULL, nothing read or written
    assert prove_d(eng, None, None, None, 0, 0, None, None, None) == 0
    assert prove_h(eng, None, None, None, 0, 0, None, None) == 0
    assert ver_d(eng, None, None, None, 0, 0, None, None) == 0
    assert ver_h(eng, None, None, None, 0, 0, None) == 0
    assert grp_d(eng, None, None, None, 0, 0, None, None, None) == 0
    n = np.full(2, 0x77, dtype=np.uint32)
    assert find_h(eng, None, None, None, 0, T, None, 2, None, None, None, None, _p(n[:1])) == 0
    assert n.tolist() == [0, 0x77]
    # a count beyond one launch
    assert ver_d(eng, pb, pb, po, bound + 1, 0, pb, pb) == E_ARG and "count too large for one launch" in _err()
    assert prove_d(eng, pb, pb, po, bound + 1, 0, pb, pb, pb) == E_ARG and "count too large for one launch" in _err()
    assert buf.tolist() == [0x77] * 64   # nothing was written


def test_size_getters_answer_zero_for_what_is_not_taken():
    L = _lib()
    buf = np.full(8, 0x77, dtype=np.uint64)
    eng = _p(buf)   # never read
    good = np.array([3, 1, 5], dtype=np.uint32)
    getters = ((L.bpp_prover_serialized_outs_workspace_bytes, ()), (L.bpp_verifier_serialized_outs_workspace_bytes, ()),
               (L.bpp_verifier_serialized_grouped_outs_workspace_bytes, (4,)), (L.bpp_verify_find_outputs_outs_workspace_bytes, (2,)))
    for f, extra in getters:
        assert f(None, _p(good), 3, *extra) == 0          # no engine
        assert f(eng, None, 3, *extra) == 0               # no counts
        assert f(eng, _p(good), (0x7fffffff // 64) + 1, *extra) == 0
        for at in range(3):
            for bad in (0, 129, 0xffffffff):              # zero, and above every engine's capacity
                outs = good.copy()
                outs[at] = bad
                assert f(eng, _p(outs), 3, *extra) == 0, (f, at, bad)
    assert buf.tolist() == [0x77] * 8


def test_outs_plan_host_build(tmp_path):
    out = subprocess.run([_build("outs_plan_host_test", tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "outs_plan ok" in out.stdout
