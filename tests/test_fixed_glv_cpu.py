"""CPU: the windows of the fixed-generator tables (csrc/fixed_glv.hpp) and the GLV path over them (csrc/ec.hpp
glv_split_balanced) as a host build (g++) of the headers the kernels compile, against Python integers and against plain
double-and-add (tests/host/fixed_glv_host_test.cpp): the balanced split, the window layouts of all three curves and their
digit recoding, and the two-phase sum with the endomorphism applied once to the accumulator."""

import os
import random
import subprocess

import pytest

import mulvec_cases as M
from glv_cases import HALF_MAX, R, Z2, edges as _edges, recode_halves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("BPP_HOST_SANITIZE") else []

assert R == Z2 * Z2 - Z2 + 1 and HALF_MAX < 2 ** 126.43


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fixed_glv") / ("bpp_fixed_glv_host_test" + ("_san" if SANITIZE else "")))
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + SANITIZE + ["-o", out, os.path.join(ROOT, "tests", "host", "fixed_glv_host_test.cpp")])
    return out


def _run(exe, args, chunk=2000):
    """the tool's output lines for `args[0:k]` (mode and its parameters) + the items args[k:], a chunk at a time"""
    head, items = args
    lines = []
    for off in range(0, len(items), chunk):
        lines += subprocess.check_output([exe] + head + items[off:off + chunk]).decode().splitlines()
    return lines


def test_balanced_split_matches_integers(exe):
    rng = random.Random(21)
    ks = _edges() + [rng.randrange(R) for _ in range(100000)]
    ks += [rng.randrange(Z2 // 2) * Z2 + d for d in (0, 1, Z2 - 1, Z2 // 2, Z2 // 2 + 1) for _ in range(200)]
    ks = [k for k in ks if k < R]
    out = _run(exe, (["split"], ["%064x" % k for k in ks]))
    assert len(out) == len(ks)
    big1 = big2 = 0
    negs = [0, 0]
    for k, line in zip(ks, out):
        s1, k1, s2, k2 = line.split()
        k1, k2 = int(k1, 16), int(k2, 16)
        v = (-k1 if s1 == "1" else k1) + (-k2 if s2 == "1" else k2) * Z2
        assert (v - k) % R == 0, hex(k)
        assert k1 <= HALF_MAX and k2 <= HALF_MAX, hex(k)
        big1, big2 = max(big1, k1), max(big2, k2)
        negs[0] += s1 == "1"
        negs[1] += s2 == "1"
    # the largest halves that occur: (r - 1) / 2 = (z^2 / 2 - 1) z^2 + z^2 / 2, so the quotient never exceeds z^2 / 2 - 1
    # after the fold either -- one below the bound the layouts are sized for
    assert big1 == Z2 // 2 and big2 == Z2 // 2 - 1
    assert min(negs) > 10000


def _layout(exe, c):
    out = subprocess.check_output([exe, "layout", str(c)]).decode().splitlines()
    W, top, per_f = (int(x) for x in out[0].split())
    wins = [tuple(int(x) for x in line.split()) for line in out[1:1 + W]]
    return W, top, per_f, wins, int(out[1 + W], 16)


@pytest.mark.parametrize("c", [10, 13, 16, 17])   # glv_cases.RECODE_WINDOW_BITS
def test_layout_and_recoding(exe, c):
    W, top, per_f, wins, bias = _layout(exe, c)
    assert W == ((255 - 1) // c + 1) // 2
    widths = [w for w, _, _ in wins[:-1]]
    offs = [o for _, o, _ in wins]
    assert wins[-1][0] == 0 and offs == [sum(widths[:j]) for j in range(W)]
    assert [e for _, _, e in wins] == [sum(1 << (w - 1) for w in widths[:j]) for j in range(W)]
    assert bias == sum(1 << (o + w - 1) for w, o, _ in wins[:-1])
    assert per_f == sum(1 << (w - 1) for w in widths) + top
    assert top == (HALF_MAX + bias) >> offs[-1]      # the largest half lands on the last entry of the top window
    if c == 17:
        assert (widths, top, per_f) == ([18, 18, 18, 18, 18, 19], 176407, 1093911)
        assert per_f * 2050 * 96 < 220e9             # the table at (64, 16)
    if c == 16:
        assert (widths, top, per_f) == ([16] * 7, 22051, 251427)
    hs = recode_halves(c, wins)
    out = _run(exe, (["recode", str(c)], ["%032x" % h for h in hs]))
    assert len(out) == len(hs)
    for h, line in zip(hs, out):
        d = [int(x) for x in line.split()]
        assert len(d) == W
        assert sum(dj << o for dj, o in zip(d, offs)) == h, hex(h)
        assert all(-(1 << (w - 1)) <= dj < (1 << (w - 1)) for dj, w in zip(d, widths)), hex(h)
        assert 0 <= d[-1] <= top, hex(h)


@pytest.mark.parametrize("c", [2, 3, 4, 13, 16])   # 2 and 3: more than 64 windows
@pytest.mark.parametrize("curve", ["secp256k1", "ed25519"])
def test_uniform_layout_and_recoding(exe, curve, c):
    """win_layout_uniform against mulvec_cases' restatement, and win_biased<10> / win_next_digit<10> on whole scalars"""
    sh = M.Shape(curve, 2, 2, c)
    r, half = sh.r, 1 << (c - 1)
    W, top, per_f, wins, bias = _layout(exe, "%d@%s" % (c, curve))
    assert W == sh.W == (r.bit_length() - 1) // c + 1 and (W > 64) == (c < 4)
    assert wins == [(c if j + 1 < W else 0, c * j, j * half) for j in range(W)]
    assert bias == sum(half << (c * j) for j in range(W - 1))
    assert top == sh.top == (r - 1 + bias) >> (c * (W - 1))
    assert per_f == (W - 1) * half + top
    offs = [c * j for j in range(W)]
    rng = random.Random(29 + c)
    ks = [k for k, _ in M.digit_scalars(curve, c)] + [0, 1, r - 1] + [rng.randrange(r) for _ in range(5000)]
    out = _run(exe, (["recode", "%d@%s" % (c, curve)], ["%064x" % k for k in ks]), chunk=1000)
    assert len(out) == len(ks)
    tops = set()
    for k, line in zip(ks, out):
        d = [int(x) for x in line.split()]
        assert d == M.recode_uniform(k, c, W), hex(k)
        assert sum(dj << o for dj, o in zip(d, offs)) == k, hex(k)
        assert all(-half <= dj < half for dj in d[:-1]), hex(k)
        assert 0 <= d[-1] <= top, hex(k)
        tops.add(d[-1])
    assert top in tops   # r - 1 reaches it


def test_table_bytes_fall_with_window_bits(exe):
    """bench.py retries narrower windows on an out-of-memory code: a narrower window must never need more table"""
    per_f = [_layout(exe, c)[2] for c in range(2, 19)]
    assert all(a <= b for a, b in zip(per_f, per_f[1:])), per_f


def test_two_phase_sum_is_the_scalar_multiple(exe):
    """phase-1 sum (k2 halves, negated), X <- beta X, phase-2 sum (k1 halves) == k F by double-and-add, in affine form;
    neighbouring scalars are also summed in one accumulator, which is where P + P, P - P and a sum that passes through
    infinity between the phases occur.  The kernel's form for a proof's left-over entries -- psi applied to each k2 entry,
    x <- beta x, instead of to the accumulator -- is held to the same k F."""
    rng = random.Random(23)
    ks = _edges()
    # pairs (neighbours): equal small scalars -> P + P in phase 2; k, r - k -> P - P; the same with only k2 halves
    # (multiples of z^2) -> in phase 1, and the accumulator is infinity when psi is applied
    for d in (1, 3, 5):
        ks += [d, d, R - d, d * Z2, d * Z2, R - d * Z2, d, 0, R - d, 0, 0]
    ks += [rng.randrange(R) for _ in range(140)]
    out = subprocess.check_output([exe, "group", "4"] + ["%064x" % k for k in ks]).decode().split()
    assert out[0] == "ok" and int(out[1]) == 3 * len(ks) - 1   # alone, alone in the left-over form, with the next one
    assert int(out[3]) >= 6 and int(out[5]) >= 6, out   # P + P and P - P were met
