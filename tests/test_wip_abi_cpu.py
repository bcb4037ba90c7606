"""CPU: the WIP seam (bpp_wip_prove_batch_device, bpp_wip_verify_batch_device, their size calls and host forms) is
declared, exported, bound, present in the Rust FFI and under the guard shim; its header block cites the reference sites;
its usage errors are return codes that write nothing; the Python wrappers exist; and the shared case builder
(tests/wip_cases.py) is itself right: with the shadow group of pyref every case proves and verifies to the identity and
every single-field tamper the GPU tests use does not.  No GPU needed: nothing here reaches a device."""

import ctypes
import os
import re

import numpy as np
import pytest

import pyref as P
import wip_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bpp_wip_prover_workspace_bytes", "bpp_wip_prove_batch_device", "bpp_wip_verifier_workspace_bytes",
           "bpp_wip_verify_batch_device", "bpp_wip_prove_batch", "bpp_wip_verify_batch")
SENTINEL = 0x7777777777777777


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
    block = raw[raw.index("the weighted inner product argument as a seam"):raw.index("bpp_wip_verify_batch(")]
    for site in ("src/weighted_inner_product_proof.rs:36-227", ":238-328", ":330-382"):
        assert site in block, site


def test_entries_run_under_the_guard():
    import test_abi_guard_cpu as G
    entries = G._entry_points(open(os.path.join(ROOT, "bulletproofsplus_amd", "csrc", "capi.hip")).read())
    for s in SYMBOLS:
        assert s in entries and any(shim in entries[s] for shim in G.SHIMS), s


def _bufs():
    buf = np.full(256, SENTINEL, dtype=np.uint64)
    return buf, buf.ctypes.data_as(ctypes.c_void_p)


def test_size_calls_return_zero_for_arguments_not_taken():
    L = _lib()
    assert L.bpp_wip_prover_workspace_bytes(None, 4) == 0
    assert L.bpp_wip_verifier_workspace_bytes(None, 4, 1) == 0
    assert L.bpp_wip_verifier_workspace_bytes(None, 4, 65) == 0


def test_null_and_flag_misuse_are_errors_that_write_nothing():
    L = _lib()
    buf, pb = _bufs()
    key = bytes(32)
    fake = ctypes.c_void_p(16)   # a non-null engine handle that is never dereferenced: the checks below come first
    # NULL engine / NULL required pointers
    assert L.bpp_wip_prove_batch_device(None, pb, pb, pb, pb, 1, 0, 0, None, None, 0, None, pb, pb, None, pb, 1 << 20, None) < 0
    assert "null" in L.bpp_last_error().decode()
    assert L.bpp_wip_verify_batch_device(None, pb, pb, pb, pb, 0, 1, 0, None, None, pb, pb, 1 << 20, None, None, None) < 0
    assert "null" in L.bpp_last_error().decode()
    assert L.bpp_wip_prove_batch(None, pb, pb, pb, pb, 1, 0, 0, None, None, 0, None, pb, pb, None) < 0
    assert L.bpp_wip_verify_batch(None, pb, pb, pb, pb, 0, 1, 0, None, None, pb, None, None) < 0
    assert L.bpp_wip_prove_batch_device(fake, None, pb, pb, pb, 1, 0, 0, None, None, 0, None, pb, pb, None, pb, 1 << 20, None) < 0
    assert L.bpp_wip_verify_batch_device(fake, pb, pb, pb, None, 0, 1, 0, None, None, pb, pb, 1 << 20, None, None, None) < 0
    # count = 0 still checks its arguments, and NULL everything with count = 0 is an error, not a crash
    assert L.bpp_wip_prove_batch_device(None, None, None, None, None, 0, 0, 0, None, None, 0, None, None, None, None, None, 0, None) < 0
    # nv = 65
    assert L.bpp_wip_prove_batch_device(fake, pb, pb, pb, pb, 1, 65, 0, None, None, 0, None, pb, pb, None, pb, 1 << 20, None) < 0
    assert "nv" in L.bpp_last_error().decode()
    assert L.bpp_wip_verify_batch_device(fake, pb, pb, pb, pb, 65, 1, 0, None, None, pb, pb, 1 << 20, None, None, None) < 0
    assert "nv" in L.bpp_last_error().decode()
    # unknown flag
    assert L.bpp_wip_prove_batch_device(fake, pb, pb, pb, pb, 1, 0, 2, None, None, 0, None, pb, pb, None, pb, 1 << 20, None) < 0
    assert "flag" in L.bpp_last_error().decode()
    assert L.bpp_wip_verify_batch_device(fake, pb, pb, pb, pb, 0, 1, 4, None, None, pb, pb, 1 << 20, None, None, None) < 0
    assert "flag" in L.bpp_last_error().decode()
    # the transcript flag without the states
    assert L.bpp_wip_prove_batch_device(fake, pb, pb, pb, pb, 1, 0, 1, None, None, 0, None, pb, pb, None, pb, 1 << 20, None) < 0
    assert "transcript" in L.bpp_last_error().decode().lower()
    assert L.bpp_wip_verify_batch_device(fake, pb, pb, pb, pb, 0, 1, 1, None, None, pb, pb, 1 << 20, None, None, None) < 0
    # blinding without the transcript flag; both sources
    assert L.bpp_wip_prove_batch_device(fake, pb, pb, pb, pb, 1, 0, 0, None, key, 0, None, pb, pb, None, pb, 1 << 20, None) < 0
    assert "blinding" in L.bpp_last_error().decode()
    assert L.bpp_wip_prove_batch_device(fake, pb, pb, pb, pb, 1, 0, 0, None, None, 0, pb, pb, pb, None, pb, 1 << 20, None) < 0
    assert L.bpp_wip_prove_batch_device(fake, pb, pb, pb, pb, 1, 0, 1, pb, key, 0, pb, pb, pb, None, pb, 1 << 20, None) < 0
    assert "both" in L.bpp_last_error().decode()
    assert (buf == SENTINEL).all()


def test_python_wrappers_exist():
    import bulletproofsplus_amd as B
    for name in ("wip_prover_workspace_bytes", "wip_prove_device", "wip_prove_batch", "wip_verifier_workspace_bytes",
                 "wip_verify_device", "wip_verify_batch"):
        assert callable(getattr(B.BatchVerifier, name)), name
    assert callable(B.WeightedInnerProductProof.prove) and callable(B.WeightedInnerProductProof.verify)


def test_power_vector_check_is_a_value_error():
    from bulletproofsplus_amd import api

    class A:
        curve = api.SECP256K1

    r = api.FR_ORDER[api.SECP256K1]
    y = 12345
    good = [pow(y, i + 1, r) for i in range(8)]
    assert api._wip_y(A, good, 8) == y
    assert api._wip_y(A, [api.scalar_to_wire(x) for x in good], 8) == y
    for bad in (good[:-1] + [good[-1] + 1], [1] + good[:-1], good[:7]):
        with pytest.raises(ValueError):
            api._wip_y(A, bad, 8)


@pytest.mark.parametrize("cname", ["secp256k1", "bls12_381"])
def test_builder_cases_prove_and_verify_with_the_shadow_group(cname):
    G = P.make_group(cname, True)
    for n in (2, 8, 32):
        for nv in (0, 1, 3):
            pk = P.PublicKey(G, n)
            c = W.random_case(pk, nv, 1000 * n + nv, zero_ends=(nv == 1), over_r=(nv == 3))
            pf = c.prove()
            assert G.is_zero(c.mulvec(pf).calculate()), (n, nv)
            for t in W.TAMPERS:
                if nv == 0 and t in ("V0", "Vc0"):
                    continue
                q, ov = W.tampered(c, pf, t)
                assert not G.is_zero(c.mulvec(q, **ov).calculate()), (n, nv, t)


@pytest.mark.parametrize("cname", ["secp256k1", "bls12_381"])
@pytest.mark.parametrize("shape", [(8, 1), (4, 4)])
def test_range_exponents_restate_the_range_statement(cname, shape):
    n, m = shape
    G = P.make_group(cname, True)
    pk = P.PublicKey(G, n * m)
    c, rp = W.range_case(pk, n, [(1 << n) - 1 - j for j in range(m)], [11 + 7 * j for j in range(m)])
    pf = c.prove()
    # the seam's prover input reproduces the range prover's WIP proof ...
    assert (pf.L_vec, pf.R_vec, pf.A, pf.B) == (rp.proof.L_vec, rp.proof.R_vec, rp.proof.A, rp.proof.B)
    assert (pf.r_prime, pf.s_prime, pf.d_prime) == (rp.proof.r_prime, rp.proof.s_prime, rp.proof.d_prime)
    # ... and the seam's statement verifies it
    assert G.is_zero(c.mulvec(pf).calculate())
    assert rp.verify(pk, n, c.V)
    q, ov = W.tampered(c, pf, "Hc0")
    assert not G.is_zero(c.mulvec(q, **ov).calculate())


def test_cpp_mirror_members_compile(tmp_path):
    """include/bpp_amd.hpp: WeightedInnerProductProof::prove / verify compile and link against the library"""
    import subprocess
    exe = str(tmp_path / "wip_mirror_main")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "wip_mirror_main.cpp"),
                           "-L" + os.path.join(ROOT, "bulletproofsplus_amd"), "-lbpp_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "bulletproofsplus_amd")])
    assert os.path.exists(exe)
