"""CPU: the commitment walk of k_commit_batch (csrc/commit_walk.hpp) through its host build
(tests/host/commit_walk_host_test.cpp): over a host-built table of g and h = 2 g in the layout of the verifier's window
tables, the walk's sum equals double-and-add of s g + gamma h -- s the amount itself (BPP_PROVE_AMOUNT64) or the reference's
new(v as i32) (src/range/prover.rs:37), which makes v = 2^31 a full-width negative scalar.  The amounts 2^j and 2^j - 1 put
a one and a run of ones across every window boundary at any width; the gammas sit at the ends and the middle of the scalar
field.  With h = 2 g the pairs (2, 1) and (2, r - 1) are P + P and P - P inside the walk: the program counts both."""

import os
import random
import re
import subprocess

import pytest

import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# BPP_HOST_SANITIZE=1: host builds under ASan + UBSan (see tests/test_host_arith_cpu.py)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("BPP_HOST_SANITIZE") else []

CURVES = {"bls12_381": 0, "secp256k1": 1, "ed25519": 2}


def amounts():
    """{2^j, 2^j - 1 : j = 0..64} clipped to 64 bits"""
    return sorted({min(x, (1 << 64) - 1) for j in range(65) for x in (1 << j, (1 << j) - 1)})


def gammas(r, seed):
    rng = random.Random(seed)
    return [0, 1, 2, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2] + [rng.randrange(r) for _ in range(8)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host") / "bpp_commit_walk_host_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + SANITIZE + ["-o", exe, os.path.join(ROOT, "tests", "host", "commit_walk_host_test.cpp")])
    return exe


@pytest.mark.parametrize("amount64", [0, 1])
@pytest.mark.parametrize("window_bits", [5, 13])
@pytest.mark.parametrize("curve", ["bls12_381", "secp256k1", "ed25519"])
def test_walk_equals_double_and_add(harness, curve, window_bits, amount64):
    r = P.CURVES[curve]["r"]
    vs, gs = amounts(), gammas(r, 20240 + CURVES[curve])
    assert len(vs) == 128 and (1 << 31) in vs and (1 << 64) - 1 in vs and 2 in vs
    out = subprocess.run([harness, str(CURVES[curve]), str(window_bits), str(amount64), str(len(vs))] +
                         ["%016x" % v for v in vs] + ["%064x" % g for g in gs], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.fullmatch(r"ok (\d+) additions (\d+) doublings (\d+) cancellations (\d+)\n", out.stdout)
    assert m, out.stdout
    sums, additions, doublings, cancellations = map(int, m.groups())
    print(curve, window_bits, amount64, out.stdout.strip())
    assert sums == len(vs) * len(gs) and additions > sums
    assert doublings > 0 and cancellations > 0


def test_fe_from_u64_at_the_limb_boundaries(harness):
    """csrc/field.hpp fe_from_u64 (30-bit limbs: a u64 spans three): every 2^j, 2^j - 1, and the values around the limb
    boundaries 2^30 and 2^60, on the three scalar fields"""
    vs = set(amounts())
    for b in (30, 60):
        vs |= {(1 << b) - 2, (1 << b) + 1, (1 << b) | 1 | (1 << (b - 1)), ((1 << b) - 1) << 1 & ((1 << 64) - 1)}
    vs |= {0x0123456789abcdef, 0xfedcba9876543210, (1 << 64) - 2}
    out = subprocess.run([harness, "u64"] + ["%016x" % v for v in sorted(vs)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout == "ok u64 %d\n" % len(vs), out.stdout + out.stderr
