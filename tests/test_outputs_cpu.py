"""CPU: the three per-output functions and the lane arithmetic of the per-output tag test (csrc/output_terms.hpp) through
their host build (tests/host/output_terms_host_test.cpp: the code k_outputs_make, k_out_tags and k_out_confirm run).

Masks, pads and tags are held against hashlib (output_cases), the lanes against a plain enumeration
(output_cases.tag_lanes).  BPP_HOST_SANITIZE=1 builds the program under ASan + UBSan (a stand-alone binary, like the other
host tests)."""

import hashlib
import subprocess

import pytest

import find_cases as FC
import output_cases as OC
import recover_cases as RC
import tag_cases as TC
from test_host_arith_cpu import _build

CURVES = ("bls12_381", "secp256k1", "ed25519")
KEYS = [bytes(32), b"\xff" * 32, hashlib.sha256(b"a recipient").digest(), hashlib.sha256(b"another recipient").digest()]
INDICES = [0, (1 << 32) - 1, 1 << 32, (1 << 64) - 1]
PLACES = [0, 1, 15, (1 << 32) - 1]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build("output_terms_host_test", tmp_path_factory.mktemp("host"), "-O2")


def _terms(harness, tmp_path, cases):
    f = tmp_path / "in.txt"
    f.write_text("".join("%d %s %d %d\n" % (c, k.hex(), i, j) for c, k, i, j in cases))
    out = subprocess.run([harness, "terms", str(f)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [line.split() for line in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    return [(int(m, 16), int(p, 16), int(t, 16)) for m, p, t in rows]


@pytest.mark.parametrize("cid", range(3))
def test_the_three_functions_are_the_hashes(harness, tmp_path, cid):
    """all-zero, all-ones and two other keys; idx on both sides of 2^32 and at both ends of u64; j in 0, 1, 15, 2^32 - 1"""
    r = RC.ORDER[CURVES[cid]]
    cases = [(cid, k, i, j) for k in KEYS for i in INDICES for j in PLACES]
    got = _terms(harness, tmp_path, cases)
    want = [(OC.mask(k, i, j, r), OC.pad(k, i, j), OC.tag(k, i, j)) for _, k, i, j in cases]
    assert got == want
    assert all(0 < m < r for m, _, _ in got)
    # all values distinct over the corpus (the tag is one byte: not one constant)
    assert len({m for m, _, _ in got}) == len(cases) and len({p for _, p, _ in got}) == len(cases)
    assert len({t for _, _, t in got}) > 16
    for (_, k, i, j), (m, p, t) in zip(cases, got):
        # the mask is no blinding slot of the same (idx, slot = j)
        assert m != OC.blinding_slot(k, i, j, r)
        # j = 0: the pad and the tag of the single-output calls, byte for byte
        if j == 0:
            assert p == FC.pad(k, i) and t == TC.tag(k, i)
        else:
            assert p != FC.pad(k, i)


def test_the_construction_is_the_stated_one():
    """output_cases itself against the issue's formulas, written out"""
    k, i, j = KEYS[2], (1 << 40) + 7, 3
    r = RC.ORDER["secp256k1"]
    blk = lambda tag4, h: hashlib.sha256(k + tag4 + i.to_bytes(8, "little") + j.to_bytes(4, "little") + h.to_bytes(4, "little")).digest()
    c0, c1 = int.from_bytes(blk(b"bppm", 0), "little"), int.from_bytes(blk(b"bppm", 1), "little")
    assert OC.mask(k, i, j, r) == (c0 + (c1 << 256)) % r
    assert OC.pad(k, i, j) == int.from_bytes(blk(b"bppa", 0)[:8], "little")
    assert OC.tag(k, i, j) == blk(b"bppt", 0)[0]


@pytest.mark.parametrize("m_c", (1, 2, 4, 16))
def test_tag_test_lanes_against_an_enumeration(harness, m_c):
    """class output counts 1, 63, 64, 65, 255, 256, 257, 513 (where m_c divides them, else the next multiple), under one
    key and under three: every pair on exactly one lane, (p, j) = (x / m_c, x % m_c), no tile across two keys"""
    logm = m_c.bit_length() - 1
    for outs in (1, 63, 64, 65, 255, 256, 257, 513):
        count_c = -(-outs // m_c)
        for n_keys in (1, 3):
            out = subprocess.run([harness, "lanes", str(n_keys), str(count_c), str(logm)], capture_output=True, text=True)
            assert out.returncode == 0, out.stdout + out.stderr
            lines = out.stdout.splitlines()
            tiles, per_key, n = (int(x) for x in lines[0].split())
            assert n == count_c * m_c and per_key == -(-n // OC.TILE) and tiles == n_keys * per_key
            got = [tuple(int(x) for x in line.split()) for line in lines[1:]]
            assert got == OC.tag_lanes(n_keys, count_c, m_c)
            assert len(got) == n_keys * n
