"""CPU: the view tag and the candidate list's index arithmetic (csrc/find_terms.hpp) through their host build
(tests/host/view_tag_host_test.cpp: the code k_view_tags, k_find_tags and k_find_list run).

The tag is held against hashlib (tag_cases.tag), the candidate list against a prefix sum (tag_cases.candidate_list, which
is find_cases.compact over the key-major flags).  BPP_HOST_SANITIZE=1 builds the program under ASan + UBSan (a stand-alone
binary, like the other host tests)."""

import hashlib
import random
import subprocess

import pytest

import find_cases as FC
import tag_cases as TC
from test_host_arith_cpu import _build

KEYS = [bytes(32), b"\xff" * 32, hashlib.sha256(b"a view key").digest()]
RNG = random.Random(7500)
INDICES = [0, (1 << 32) - 1, 1 << 32, (1 << 64) - 1] + [RNG.randrange(1 << 64) for _ in range(12)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build("view_tag_host_test", tmp_path_factory.mktemp("host"), "-O2")


def _run(harness, tmp_path, args, text):
    f = tmp_path / "in.txt"
    f.write_text(text)
    out = subprocess.run([harness] + args + [str(f)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def test_tag_is_the_first_byte_of_the_tagged_hash(harness, tmp_path):
    """the all-zero, the all-ones and a random key; indices 0, 2^32 - 1, 2^32, 2^64 - 1 and random ones"""
    cases = [(k, i) for k in KEYS for i in INDICES]
    got = _run(harness, tmp_path, ["tag"], "".join("%s %d\n" % (k.hex(), i) for k, i in cases))
    assert [int(x, 16) for x in got] == [TC.tag(k, i) for k, i in cases]
    assert len(set(got)) > 16   # one byte each, and not one constant
    # a third domain: neither the pad's block nor a blinding slot's
    k, i = KEYS[2], INDICES[5]
    want = hashlib.sha256(k + b"bppt" + i.to_bytes(8, "little") + bytes(8)).digest()
    assert TC.tag(k, i) == want[0]
    assert want[:8] != FC.pad(k, i).to_bytes(8, "little")
    assert want != hashlib.sha256(k + b"bppb" + i.to_bytes(8, "little") + bytes(8)).digest()


def test_candidate_list_against_a_prefix_sum(harness, tmp_path):
    """no pair, one pair, one key and many, rows that end inside a tile, on a tile edge and one beyond; candidates on both
    sides of a round and of a tile boundary, a whole tile of them, a key with none; every pair a candidate; random
    densities"""
    T = FC.TILE
    rng = random.Random(7600)

    def rows(n_keys, count, at):
        f = [[0] * count for _ in range(n_keys)]
        for j, p in at:
            f[j][p] = 1
        return f
    shapes = [rows(1, 1, []), rows(1, 1, [(0, 0)]), rows(3, 1, [(0, 0), (2, 0)]), rows(1, 63, [(0, 0), (0, 62)]),
              rows(2, T, [(0, 0), (0, 63), (0, 64), (0, T - 1), (1, 0), (1, T - 1)]),
              rows(3, T + 1, [(0, T - 1), (0, T), (2, T)]), rows(3, 683, [(1, p) for p in range(341, 597)] + [(0, 0), (2, 682)]),
              [[1] * (2 * T + 5) for _ in range(3)], [[0] * (T + 7) for _ in range(2)]]
    for dens in (0.004, 0.3, 0.9):
        n_keys, count = rng.randrange(2, 6), rng.randrange(T + 1, 4 * T)
        shapes.append([[1 if rng.random() < dens else 0 for _ in range(count)] for _ in range(n_keys)])
    for flags in shapes:
        n_keys, count = len(flags), len(flags[0])
        got = _run(harness, tmp_path, ["list", str(n_keys), str(count)], "".join(str(f) for row in flags for f in row) + "\n")
        tiles, cands = (int(x) for x in got[0].split())
        want_n, want = TC.candidate_list(flags)
        assert tiles == n_keys * -(-count // T) and cands == want_n == sum(map(sum, flags))
        assert [int(x) for x in got[1:]] == want
