"""CPU: the field operations of csrc/field.hpp on RAW limb images at their stated bounds -- all-ones limbs, values up to
8 p, unreduced sums, the _io forms, the two-product fe_mul_add, the inverses -- as a host build (g++) of
csrc/field_raw_ops.hpp (tests/host/field_raw_host_test.cpp), against Python integers.  The cases and the reference are
those of tests/field_cases.py; test_gpu_field_raw.py runs the same on the device."""

import os
import subprocess

import numpy as np
import pytest

import field_cases as FC
import madd_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# BPP_HOST_SANITIZE=1: the same build under AddressSanitizer + UndefinedBehaviorSanitizer
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("BPP_HOST_SANITIZE") else []


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("field_raw") / ("bpp_field_raw_host_test" + ("_san" if SANITIZE else "")))
    subprocess.check_call(["g++", "-O1", "-std=c++17"] + SANITIZE + ["-o", out, os.path.join(ROOT, "tests", "host", "field_raw_host_test.cpp")])
    return out


def host_runner(exe):
    def run(f, code, a, b, c, d):
        n = a.shape[0]
        head = np.array([0, f.cid, f.idx, code, n], dtype=np.uint32)
        blob = b"".join(x.tobytes() for x in (head, a, b, c, d))
        out = subprocess.run([exe], input=blob, stdout=subprocess.PIPE, check=True).stdout
        return np.frombuffer(out, dtype=np.uint32).reshape(n, 2 * f.NL)
    return run


@pytest.mark.parametrize("fname", list(FC.FIELDS))
def test_raw_field_ops_match_integers(exe, fname):
    FC.run_and_check(fname, host_runner(exe))


def test_mul_add_of_all_ones_limbs_on_the_13_limb_field(exe):
    """a = b = c = d = 2^360 - 1 (limbs 0..11 all-ones, limb 12 zero: normalised, below p): the 26 plain products of a
    middle column, each (2^30 - 1)^2, do not fit one 64-bit accumulator -- fe_mul_add keeps two chains there.  With one
    chain the result was not congruent to a b + c d."""
    f = FC.FIELDS["bls12_381_fp"]
    v = FC.OVERFLOW_PROBE
    assert v < f.p and all(l == FC.LIMB_MASK for l in FC.limbs(v, f.NL)[:12]) and FC.limbs(v, f.NL)[12] == 0
    assert any(c.op == "mul_add" and (v, v, v, v) in zip(c.A, c.B, c.C, c.D) for c in FC.cases(f.name))
    case = FC.Case("mul_add", FC.OP_CODE["mul_add"], [v], [v], [v], [v])
    FC.check(f, case, host_runner(exe)(f, case.code, *FC.operand_arrays(f, case)))
    # 26 products of all-ones limbs overflow 64 bits, 13 do not: the bound the two chains rest on
    assert 26 * FC.LIMB_MASK ** 2 >= 1 << 64 > 15 * FC.LIMB_MASK ** 2 + (1 << 36)


@pytest.mark.parametrize("curve", list(MC.CURVES))
def test_lazy_mixed_addition_on_raw_accumulators(exe, curve):
    """xyzz_madd_lazy on accumulators in every representation its invariant allows (tests/madd_cases.py), host build"""
    c = MC.cases(curve)
    f = FC.FIELDS[MC.CURVES[curve]]
    n = len(c.want)
    head = np.array([1, f.cid, 0, 0, n], dtype=np.uint32)
    blob = b"".join(x.tobytes() for x in (head, c.acc, c.q, c.neg))
    out = subprocess.run([exe], input=blob, stdout=subprocess.PIPE, check=True).stdout
    MC.check(curve, np.frombuffer(out, dtype=np.uint32).reshape(n, 4, f.NL))
