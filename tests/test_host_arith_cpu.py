"""CPU: host builds (g++) of the device headers' arithmetic that has no oracle counterpart because it is an ENGINE
optimisation, not reference behaviour: the lazy (unreduced) XYZZ mixed addition against the eager one with every
intermediate bound asserted (tests/host/lazy_host_test.cpp), and the GLV scalar split of the BLS12-381 proof-point MSM
(tests/host/glv_host_test.cpp) against Python integers."""

import os
import subprocess

import pyref as P
from glv_cases import SECP_LAMBDA, bls_split_scalars, secp_split_scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# BPP_HOST_SANITIZE=1: the same host builds under AddressSanitizer + UndefinedBehaviorSanitizer (the GPU pool offers no
# sanitizer, so the device headers' arithmetic gets its sanitizer run here, on the CPU build)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("BPP_HOST_SANITIZE") else []


def _build(name, tmp_path, opt="-O1"):
    exe = str(tmp_path / ("bpp_" + name + ("_san" if SANITIZE else "")))
    subprocess.check_call(["g++", opt, "-std=c++17"] + SANITIZE + ["-o", exe, os.path.join(ROOT, "tests", "host", name + ".cpp")])
    return exe


def test_lazy_mixed_addition_bounds_and_values(tmp_path):
    out = subprocess.check_output([_build("lazy_host_test", tmp_path)]).decode()
    assert "ok bls12_381" in out and "ok secp256k1" in out


def test_edwards_lazy_mixed_addition(tmp_path):
    out = subprocess.check_output([_build("ed_lazy_host_test", tmp_path)]).decode()
    assert "ok ed25519" in out


def test_glv_split_matches_integers(tmp_path):
    exe = _build("glv_host_test", tmp_path, "-O2")
    r = P.BLS12_381["r"]
    z2 = 0xd201000000010000 ** 2
    ks = bls_split_scalars()
    assert len(ks) > 3000 and all(k < r for k in ks)
    for off in range(0, len(ks), 500):
        chunk = ks[off:off + 500]
        out = subprocess.check_output([exe] + ["%064x" % k for k in chunk]).decode().split("\n")
        for k, line in zip(chunk, out):
            k1, k2 = (int(x, 16) for x in line.split())
            assert (k1, k2) == (k % z2, k // z2), hex(k)
            assert k1 < (1 << 128) and k2 < (1 << 128)


def test_glv_split_secp256k1_signed(tmp_path):
    """k == (+-k1) + (+-k2) lambda mod n with both magnitudes below 2^128 -- random scalars and the edges (0, 1, n - 1,
    lambda, n - lambda, the middle of the range, values that make either half negative)"""
    exe = _build("glv_host_test", tmp_path, "-O2")
    n = P.SECP256K1["r"]
    lam = SECP_LAMBDA
    assert (lam * lam + lam + 1) % n == 0
    ks = secp_split_scalars()
    assert len(ks) > 4000 and all(k < n for k in ks)
    seen_neg = [0, 0]
    for off in range(0, len(ks), 500):
        chunk = ks[off:off + 500]
        out = subprocess.check_output([exe, "secp"] + ["%064x" % k for k in chunk]).decode().split("\n")
        for k, line in zip(chunk, out):
            s1, k1, s2, k2 = line.split()
            k1, k2 = int(k1, 16), int(k2, 16)
            v1 = -k1 if s1 == "1" else k1
            v2 = -k2 if s2 == "1" else k2
            assert (v1 + v2 * lam - k) % n == 0, hex(k)
            assert k1 < (1 << 128) and k2 < (1 << 128), hex(k)
            seen_neg[0] += s1 == "1"
            seen_neg[1] += s2 == "1"
    assert seen_neg[0] > 100 and seen_neg[1] > 100
