"""CPU: the pad of a sealed amount and the compaction's index arithmetic (csrc/find_terms.hpp) through their host build
(tests/host/find_host_test.cpp: the code k_amounts_seal, the two confirmation kernels, k_find_count and k_find_emit run).

The pad is held against hashlib (find_cases.pad), the hit list against a prefix sum (find_cases.compact).
BPP_HOST_SANITIZE=1 builds the program under ASan + UBSan (a stand-alone binary, like the other host tests)."""

import hashlib
import os
import random
import re
import subprocess

import pytest

import find_cases as FC
from test_host_arith_cpu import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [bytes(32), b"\xff" * 32, bytes(range(7, 39)), hashlib.sha256(b"a view key").digest()]
INDICES = [0, 1, 5, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 33) + 5, (1 << 63) + 9, (1 << 64) - 1]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build("find_host_test", tmp_path_factory.mktemp("host"), "-O2")


def _run(harness, tmp_path, args, text):
    f = tmp_path / "in.txt"
    f.write_text(text)
    out = subprocess.run([harness] + args + [str(f)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def test_pad_is_the_tagged_hash(harness, tmp_path):
    """the all-zero and the all-ones key among them; indices on both sides of 2^32 and at both ends of u64"""
    cases = [(k, i) for k in KEYS for i in INDICES]
    got = _run(harness, tmp_path, ["pad"], "".join("%s %d\n" % (k.hex(), i) for k, i in cases))
    assert [int(x, 16) for x in got] == [FC.pad(k, i) for k, i in cases]
    assert len(set(got)) == len(cases)
    # not a blinding slot: the tag differs from the slots' in one byte
    k, i = KEYS[2], INDICES[6]
    slot = hashlib.sha256(k + b"bppb" + i.to_bytes(8, "little") + bytes(8)).digest()
    assert FC.pad(k, i) != int.from_bytes(slot[:8], "little")


def test_sealing_twice_is_the_identity(harness, tmp_path):
    rng = random.Random(7100)
    amounts = [0, 1, (1 << 31) + 5, (1 << 64) - 1] + [rng.randrange(1 << 64) for _ in range(12)]
    cases = [(KEYS[n % len(KEYS)], INDICES[n % len(INDICES)], a) for n, a in enumerate(amounts)]
    got = _run(harness, tmp_path, ["seal"], "".join("%s %d %d\n" % (k.hex(), i, a) for k, i, a in cases))
    for (k, i, a), line in zip(cases, got):
        sealed, twice = (int(x) for x in line.split())
        assert sealed == a ^ FC.pad(k, i) and twice == a
    assert FC.seal(KEYS[3], FC.seal(KEYS[3], amounts, range(len(amounts))), range(len(amounts))) == amounts


def test_tile_size_matches_the_header():
    src = open(os.path.join(ROOT, "bulletproofsplus_amd", "csrc", "find_terms.hpp")).read()
    block = int(re.search(r"FIND_BLOCK = (\d+);", src).group(1))
    rounds = int(re.search(r"FIND_ROUNDS = (\d+);", src).group(1))
    assert block == 64 and block * rounds == FC.TILE


def _flags(pairs, hits):
    f = [0] * pairs
    for h in hits:
        f[h] = 1
    return f


def test_compaction_against_a_prefix_sum(harness, tmp_path):
    """empty, all set, one tile and a short last one, hits on both sides of a tile and of a round boundary, a tile with
    none, random densities; max_hits 0, 1, hits - 1, hits and above"""
    T = FC.TILE
    rng = random.Random(7200)
    shapes = [_flags(1, []), _flags(1, [0]), _flags(63, [0, 62]), _flags(T, [0, 63, 64, T - 1]), [1] * (2 * T + 1),
              _flags(3 * T + 1, [T - 1, T, 3 * T]), _flags(4 * T + 7, [0, T - 1, T, 3 * T, 4 * T + 6]), [0] * (2 * T + 5)]
    for dens in (0.01, 0.3, 0.9):
        pairs = rng.randrange(2 * T + 1, 6 * T)
        shapes.append([1 if rng.random() < dens else 0 for _ in range(pairs)])
    for flags in shapes:
        total = sum(flags)
        for max_hits in sorted({0, 1, max(total - 1, 0), total, total + 3}):
            got = _run(harness, tmp_path, ["compact", str(max_hits)], "".join(map(str, flags)) + "\n")
            tiles, hits = (int(x) for x in got[0].split())
            want_hits, want = FC.compact(flags, max_hits)
            assert tiles == -(-len(flags) // T) and hits == want_hits == total
            assert [int(x) for x in got[1:]] == want
