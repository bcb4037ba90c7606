"""CPU: the shape and digit code of the bucket-method MulVec (csrc/pip_shape.hpp, included by csrc/pippenger.hpp) in a
stand-alone host build (tests/host/pip_shape_host_test.cpp; under ASan + UBSan with BPP_HOST_SANITIZE=1).

 * geometry: the relations between the members of PipShape that the kernels rely on, for both scalar layouts the engine
   uses (GLV: 128 bits, max 2^128 - 1; edwards25519: 253 bits, max r), every window width 2..16, sizes 1 .. 2^28 - 1
 * recoding: the digits pip_digit takes from value + bias, put together again with Python integers, over values that
   reach both ends of every window's digit range
 * REGIMES: the shapes of the cases of tests/test_gpu_msm_shapes.py, with the members (S, fb, fl, cpw, the padding of
   `sorted`) that the C ABI's shape report does not carry."""

import random
import subprocess

import pytest

import pyref as P
from test_host_arith_cpu import _build

KINDS = {"glv": (128, (1 << 128) - 1), "ed": (253, P.ED25519["r"])}
WIDTHS = range(2, 17)

# (kind, n, window_bits; 0 = chosen from n) -> c, W, q, nwide, top, nbuckets, S, L, fb, fl, cpw, istride - items
REGIMES = {
    ("glv", (1 << 15) + 1, 2): (2, 64, 2, 0, 4, 130, 1, 16, 5, 8, 4097, 2),
    ("glv", (1 << 16) + 1, 2): (2, 64, 2, 0, 4, 130, 1, 32, 5, 8, 4097, 2),
    ("glv", (1 << 17) + 1, 2): (2, 64, 2, 0, 4, 130, 1, 64, 5, 8, 4097, 2),
    ("glv", 1 << 18, 12): (12, 11, 11, 7, 2048, 19456, 1, 16, 5, 8, 32768, 0),
    ("glv", 1 << 18, 15): (15, 9, 14, 2, 16384, 98304, 2, 16, 6, 2, 32768, 0),
    ("glv", 1 << 19, 13): (13, 10, 12, 8, 4096, 38912, 1, 32, 5, 4, 32768, 0),
    ("glv", (1 << 20) + 1, 0): (16, 8, 16, 0, 65536, 294912, 8, 64, 8, 1, 32769, 2),
    ("glv", 1 << 22, 0): (16, 8, 16, 0, 65536, 294912, 8, 64, 8, 1, 131072, 0),      # the benchmark's own shape
    ("ed", 33027, 2): (2, 127, 1, 126, 1, 253, 1, 16, 5, 8, 2065, 1),
    ("ed", 66053, 2): (2, 127, 1, 126, 1, 253, 1, 32, 5, 8, 2065, 3),
    ("ed", 132105, 2): (2, 127, 1, 126, 1, 253, 1, 64, 5, 8, 2065, 3),
    ("ed", 1 << 18, 12): (12, 22, 11, 11, 1024, 33792, 1, 16, 5, 4, 16384, 0),
    ("ed", 1 << 18, 15): (15, 17, 14, 15, 8192, 262144, 2, 16, 8, 1, 16384, 0),
    ("ed", 1 << 19, 13): (13, 20, 12, 13, 2048, 67584, 1, 32, 6, 2, 16384, 0),
    # the width chosen at this size is 15 (S = 2); S = 4 is the explicit width 16
    ("ed", (1 << 20) + 1, 0): (15, 17, 14, 15, 8192, 262144, 2, 64, 8, 1, 16385, 3),
    ("ed", (1 << 20) + 1, 16): (16, 16, 15, 13, 16384, 475136, 4, 64, 8, 1, 16385, 3),
    # the block and padding boundaries (chunk length 8): one point past a block of the sort, both sides of the size from
    # which the host-pointer MulVec takes this pipeline, chunks per window that are no multiple of the block of the bucket sums
    ("glv", 2047, 0): (8, 16, 8, 0, 256, 2176, 1, 8, 5, 4, 512, 2),
    ("glv", 2048, 0): (9, 15, 8, 8, 256, 3072, 1, 8, 5, 2, 512, 0),
    ("glv", 2049, 0): (9, 15, 8, 8, 256, 3072, 1, 8, 5, 2, 513, 2),
    ("glv", 4095, 0): (9, 15, 8, 8, 256, 3072, 1, 8, 5, 4, 1024, 2),
    ("glv", 4096, 0): (10, 13, 9, 11, 512, 6400, 1, 8, 5, 2, 1024, 0),
    ("glv", 4097, 0): (10, 13, 9, 11, 512, 6400, 1, 8, 5, 2, 1025, 2),
    ("glv", 8191, 0): (10, 13, 9, 11, 512, 6400, 1, 8, 5, 4, 2048, 2),
    ("glv", 4097, 2): (2, 64, 2, 0, 4, 130, 1, 8, 5, 8, 1025, 2),
    ("glv", 4097, 7): (7, 19, 6, 14, 64, 1088, 1, 8, 5, 8, 1025, 2),
    ("glv", 4097, 16): (16, 8, 16, 0, 65536, 294912, 8, 8, 8, 1, 1025, 2),
    ("ed", 2047, 0): (7, 37, 6, 31, 32, 2176, 1, 8, 5, 4, 256, 1),
    ("ed", 2048, 0): (8, 32, 7, 29, 64, 3904, 1, 8, 5, 2, 256, 0),
    ("ed", 2049, 0): (8, 32, 7, 29, 64, 3904, 1, 8, 5, 2, 257, 3),
    ("ed", 4095, 0): (8, 32, 7, 29, 64, 3904, 1, 8, 5, 4, 512, 1),
    ("ed", 4096, 0): (9, 29, 8, 21, 128, 6400, 1, 8, 5, 2, 512, 0),
    ("ed", 4097, 0): (9, 29, 8, 21, 128, 6400, 1, 8, 5, 2, 513, 3),
    ("ed", 8191, 0): (9, 29, 8, 21, 128, 6400, 1, 8, 5, 4, 1024, 1),
    ("ed", 4097, 2): (2, 127, 1, 126, 1, 253, 1, 8, 5, 8, 513, 3),
    ("ed", 4097, 7): (7, 37, 6, 31, 32, 2176, 1, 8, 5, 8, 513, 3),
    ("ed", 4097, 16): (16, 16, 15, 13, 16384, 475136, 4, 8, 8, 1, 513, 3),
    # the edge scalars: the sizes of the lists of glv_cases.py / of the powers of two below r
    ("glv", 3420, 0): (9, 15, 8, 8, 256, 3072, 1, 8, 5, 4, 855, 0),
    ("glv", 3420, 2): (2, 64, 2, 0, 4, 130, 1, 8, 5, 8, 855, 0),
    ("glv", 3420, 5): (5, 26, 4, 24, 16, 408, 1, 8, 5, 8, 855, 0),
    ("glv", 3420, 13): (13, 10, 12, 8, 4096, 38912, 1, 8, 5, 1, 855, 0),
    ("glv", 3420, 16): (16, 8, 16, 0, 65536, 294912, 8, 8, 8, 1, 855, 0),
    ("glv", 4031, 0): (9, 15, 8, 8, 256, 3072, 1, 8, 5, 4, 1008, 2),
    ("glv", 4031, 2): (2, 64, 2, 0, 4, 130, 1, 8, 5, 8, 1008, 2),
    ("glv", 4031, 5): (5, 26, 4, 24, 16, 408, 1, 8, 5, 8, 1008, 2),
    ("glv", 4031, 13): (13, 10, 12, 8, 4096, 38912, 1, 8, 5, 1, 1008, 2),
    ("glv", 4031, 16): (16, 8, 16, 0, 65536, 294912, 8, 8, 8, 1, 1008, 2),
    ("ed", 1012, 0): (7, 37, 6, 31, 32, 2176, 1, 8, 5, 2, 127, 0),
    ("ed", 1012, 2): (2, 127, 1, 126, 1, 253, 1, 8, 5, 8, 127, 0),
    ("ed", 1012, 5): (5, 51, 4, 49, 8, 800, 1, 8, 5, 8, 127, 0),
    ("ed", 1012, 13): (13, 20, 12, 13, 2048, 67584, 1, 8, 6, 1, 127, 0),
    ("ed", 1012, 16): (16, 16, 15, 13, 16384, 475136, 4, 8, 8, 1, 127, 0),
}
FIELDS = ("c", "W", "q", "nwide", "top", "nbuckets", "S", "L", "fb", "fl", "cpw", "pad")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build("pip_shape_host_test", tmp_path_factory.mktemp("pip_shape"), "-O2")


def run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_geometry_every_width_and_size(exe, kind):
    out = run(exe, "geometry", kind)
    assert out.returncode == 0 and out.stdout.startswith("ok geometry %s 165" % kind), out.stdout + out.stderr


def layout(exe, kind, c):
    out = run(exe, "layout", kind, c)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    W, top = (int(x) for x in lines[0].split())
    return top, [tuple(int(x) for x in lines[1 + j].split()) for j in range(W)]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_layout_is_the_even_split_of_the_bits(exe, kind):
    """the windows restated: W = ceil(bits / c) windows, the low bits % W of them one bit wider; half the range of buckets
    per signed window; the top window takes what (max + bias) leaves"""
    bits, vmax = KINDS[kind]
    for c in WIDTHS:
        top, wins = layout(exe, kind, c)
        W = -(-bits // c)
        q, nwide = bits // W, bits % W
        off = 0
        for j, (o, w, nb) in enumerate(wins):
            assert (o, w) == (off, q + (1 if j < nwide else 0)), (c, j)
            assert nb == (top if j == W - 1 else 1 << (w - 1)), (c, j)
            off += w
        assert len(wins) == W and off == bits
        bias = sum(1 << (o + w - 1) for o, w, _ in wins[:-1])
        assert top == (vmax + bias) >> wins[-1][0] and 1 <= top <= 1 << 17, c


def values(kind, wins):
    """0, 1, max, max - 1, 2^k and 2^k +- 1 for every k, a few hundred random values -- and, because 2^k - 1 carries into
    the window above, per window the two values that hold its largest and its smallest digit without a carry from below"""
    bits, vmax = KINDS[kind]
    rng = random.Random(31 + bits)
    vs = [0, 1, vmax, vmax - 1]
    for k in range(bits + 1):
        vs += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    vs += [rng.randrange(vmax + 1) for _ in range(300)]
    for o, w, _ in wins[:-1]:
        vs += [((1 << (w - 1)) - 1) << o, 1 << (o + w - 1)]
    return sorted(set(v for v in vs if 0 <= v <= vmax))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_recoding_sums_to_the_value_and_reaches_every_edge(exe, kind):
    """sum_j digit_j 2^off(j) == v; signed digits in [-nb, nb - 1], the top digit in [0, top]; over the set every window
    takes both ends of its range and 0 (the entry that is skipped)"""
    for c in WIDTHS:
        top, wins = layout(exe, kind, c)
        vs = values(kind, wins)
        out = run(exe, "recode", kind, c, *["%064x" % v for v in vs])
        assert out.returncode == 0, out.stderr
        lines = out.stdout.split("\n")
        assert len(lines) == len(vs) + 1
        seen = [set() for _ in wins]
        for v, line in zip(vs, lines):
            dg = [int(x) for x in line.split()]
            assert len(dg) == len(wins)
            assert sum(d << o for d, (o, _, _) in zip(dg, wins)) == v, (c, hex(v))
            for j, (d, (_, _, nb)) in enumerate(zip(dg, wins)):
                lo, hi = (0, top) if j == len(wins) - 1 else (-nb, nb - 1)
                assert lo <= d <= hi, (c, hex(v), j)
                if d in (lo, hi, 0):
                    seen[j].add(d)
        for j, (_, _, nb) in enumerate(wins):
            want = {0, top} if j == len(wins) - 1 else {-nb, 0, nb - 1}
            assert seen[j] == want, (c, j)


def test_regime_table(exe):
    """the shapes the GPU cases of test_gpu_msm_shapes.py stand on: chunk lengths 16 / 32 / 64 under both layouts,
    S in {1, 2, 4, 8}, fb in {5, 6, 8}, fl in {1, 2, 4, 8}, every padding of `sorted` from 0 to 3"""
    keys = sorted(REGIMES)
    out = run(exe, "table", *["%s:%d:%d" % k for k in keys])
    assert out.returncode == 0, out.stderr
    got = {k: tuple(int(x) for x in line.split()) for k, line in zip(keys, out.stdout.split("\n"))}
    assert got == REGIMES
    col = {f: i for i, f in enumerate(FIELDS)}
    for kind in KINDS:
        rows = [v for k, v in REGIMES.items() if k[0] == kind]
        assert {r[col["L"]] for r in rows} == {8, 16, 32, 64}
        assert {r[col["fl"]] for r in rows} == {1, 2, 4, 8}
        assert {5, 6, 8} <= {r[col["fb"]] for r in rows}
    assert {r[col["S"]] for r in REGIMES.values()} == {1, 2, 4, 8}
    assert {r[col["pad"]] for r in REGIMES.values()} == {0, 1, 2, 3}

