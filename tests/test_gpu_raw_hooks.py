"""-m gpu: the other two hooks of csrc/tu_debug.hip, as the DEVICE compiles what they call.
  * xyzz_madd_lazy on raw accumulator images in every representation its invariant allows (tests/madd_cases.py, which
    test_field_raw_cpu.py runs on the host build), against pyref's group law.
  * the scalar splits (csrc/ec.hpp glv_split, glv_split_balanced, glv_split_signed) and the digit recoding of the
    fixed-generator tables (csrc/fixed_glv.hpp win_biased, win_next_digit) on the edge lists the host builds are
    checked on (tests/glv_cases.py; uniform layouts: tests/mulvec_cases.py digit_scalars), against Python integers."""

import random

import numpy as np
import pytest

import glv_cases as G
import madd_cases as MC
from field_cases import FIELDS
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("curve", list(MC.CURVES))
def test_lazy_mixed_addition_on_raw_accumulators_on_device(curve):
    need_gpu()
    import bulletproofsplus_amd as B
    from bulletproofsplus_amd import _lib
    a = B.Arith.init(curve)
    c = MC.cases(curve)
    NL = FIELDS[MC.CURVES[curve]].NL
    n = len(c.want)
    assert n > 64   # more than one block
    acc, q, neg = (np.ascontiguousarray(x, dtype=np.uint32) for x in (c.acc, c.q, c.neg))
    out = np.full((n, 4, NL), 0xFFFFFFFF, dtype=np.uint32)
    assert _lib.lib().bpp_debug_madd_lazy_raw(a.handle, acc.ctypes.data, q.ctypes.data, neg.ctypes.data, n, out.ctypes.data) == 0
    MC.check(curve, out)


def _words(vals, n):
    return np.array([[(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)] for v in vals], dtype=np.uint32).reshape(len(vals), n)


def _split(curve, op, ks):
    """-> [(k1, k2, neg1, neg2)] from the device"""
    import bulletproofsplus_amd as B
    from bulletproofsplus_amd import _lib
    a = B.Arith.init(curve)
    k = _words(ks, 8)
    out = np.full((len(ks), 10), 0xFFFFFFFF, dtype=np.uint32)
    assert _lib.lib().bpp_debug_glv_op(a.handle, op, 0, k.ctypes.data, len(ks), out.ctypes.data, None) == 0
    val = lambda row: sum(int(w) << (32 * i) for i, w in enumerate(row))
    assert set(np.unique(out[:, 8:])) <= {0, 1}
    return [(val(r[0:4]), val(r[4:8]), int(r[8]), int(r[9])) for r in out]


def test_glv_split_on_device():
    need_gpu()
    ks = G.bls_split_scalars() + G.edges()
    for op in (0, 2):   # glv_split itself, and glv_split_signed, which on BLS12-381 is the same split with both signs clear
        for k, (k1, k2, n1, n2) in zip(ks, _split("bls12_381", op, ks)):
            assert (k1, k2) == (k % G.Z2, k // G.Z2) and (n1, n2) == (0, 0), hex(k)
            assert k1 < (1 << 128) and k2 < (1 << 128)


def test_balanced_split_on_device():
    need_gpu()
    rng = random.Random(21)
    ks = G.edges() + [rng.randrange(G.R) for _ in range(5000)]
    ks += [rng.randrange(G.Z2 // 2) * G.Z2 + d for d in (0, 1, G.Z2 - 1, G.Z2 // 2, G.Z2 // 2 + 1) for _ in range(200)]
    ks = [k for k in ks if k < G.R]
    big1 = big2 = 0
    negs = [0, 0]
    for k, (k1, k2, s1, s2) in zip(ks, _split("bls12_381", 1, ks)):
        v = (-k1 if s1 else k1) + (-k2 if s2 else k2) * G.Z2
        assert (v - k) % G.R == 0, hex(k)
        assert k1 <= G.HALF_MAX and k2 <= G.HALF_MAX, hex(k)
        big1, big2 = max(big1, k1), max(big2, k2)
        negs[0] += s1
        negs[1] += s2
    assert big1 == G.Z2 // 2 and big2 == G.Z2 // 2 - 1   # the largest halves that occur (test_fixed_glv_cpu.py)
    assert min(negs) > 1000


def test_signed_split_secp256k1_on_device():
    need_gpu()
    n, lam = G.SECP_N, G.SECP_LAMBDA
    ks = G.secp_split_scalars()
    seen_neg = [0, 0]
    for k, (k1, k2, s1, s2) in zip(ks, _split("secp256k1", 2, ks)):
        v1 = -k1 if s1 else k1
        v2 = -k2 if s2 else k2
        assert (v1 + v2 * lam - k) % n == 0, hex(k)
        assert k1 < (1 << 128) and k2 < (1 << 128), hex(k)
        seen_neg[0] += s1
        seen_neg[1] += s2
    assert seen_neg[0] > 100 and seen_neg[1] > 100


@pytest.mark.parametrize("c", G.RECODE_WINDOW_BITS)
def test_recoding_on_device(c):
    need_gpu()
    import bulletproofsplus_amd as B
    from bulletproofsplus_amd import _lib
    a = B.Arith.init("bls12_381")

    def recode(hs):
        h = _words(hs, 4)
        out = np.full((max(len(hs), 1), 64), 0x7FFFFFFF, dtype=np.uint32)
        lay = np.zeros(3 + 64, dtype=np.uint32)
        assert _lib.lib().bpp_debug_glv_op(a.handle, 3, c, h.ctypes.data, len(hs), out.ctypes.data, lay.ctypes.data) == 0
        return out.view(np.int32), lay

    _, lay = recode([])
    W, top = int(lay[0]), int(lay[1])
    widths = [int(w) for w in lay[3:3 + W - 1]]
    assert W == ((255 - 1) // c + 1) // 2 and int(lay[3 + W - 1]) == 0
    offs = [sum(widths[:j]) for j in range(W)]
    ents = [sum(1 << (w - 1) for w in widths[:j]) for j in range(W)]
    assert int(lay[2]) == sum(1 << (w - 1) for w in widths) + top
    wins = list(zip(widths + [0], offs, ents))
    hs = G.recode_halves(c, wins)
    out, _ = recode(hs)
    assert not out[:, W:].any()
    for h, row in zip(hs, out):
        d = [int(x) for x in row[:W]]
        assert sum(dj << o for dj, o in zip(d, offs)) == h, hex(h)
        assert all(-(1 << (w - 1)) <= dj < (1 << (w - 1)) for dj, w in zip(d, widths)), hex(h)
        assert 0 <= d[-1] <= top, hex(h)


UNIFORM_ROW = 128   # csrc/kernels.hpp VS_MAXW: the hook's row on the curves whose tables take whole scalars


@pytest.mark.parametrize("c", [3, 4, 16])
@pytest.mark.parametrize("curve", ["secp256k1", "ed25519"])
def test_recoding_on_device_uniform(curve, c):
    """the uniform layout (csrc/fixed_glv.hpp win_layout_uniform) and the recoding of whole scalars as the device
    compiles them: the identities of test_fixed_glv_cpu.py test_uniform_layout_and_recoding"""
    need_gpu()
    import bulletproofsplus_amd as B
    from bulletproofsplus_amd import _lib
    import mulvec_cases as M
    a = B.Arith.init(curve)
    sh = M.Shape(curve, 2, 2, c)
    r, W = sh.r, sh.W

    def recode(ks):
        k = _words(ks, 8)
        out = np.full((max(len(ks), 1), UNIFORM_ROW), 0x7FFFFFFF, dtype=np.uint32)
        lay = np.zeros(3 + UNIFORM_ROW, dtype=np.uint32)
        assert _lib.lib().bpp_debug_glv_op(a.handle, 3, c, k.ctypes.data, len(ks), out.ctypes.data, lay.ctypes.data) == 0
        return out.view(np.int32), lay

    _, lay = recode([])
    assert (int(lay[0]), int(lay[1])) == (W, sh.top)
    assert int(lay[2]) == (W - 1) * sh.half + sh.top
    assert [int(w) for w in lay[3:]] == [c] * (W - 1) + [0] * (UNIFORM_ROW - W + 1)
    offs = [c * j for j in range(W)]
    rng = random.Random(31 + c)
    ks = [k for k, _ in M.digit_scalars(curve, c)] + [0, 1, r - 1] + [rng.randrange(r) for _ in range(2000)]
    out, _ = recode(ks)
    assert not out[:, W:].any()
    tops = set()
    for k, row in zip(ks, out):
        d = [int(x) for x in row[:W]]
        assert d == M.recode_uniform(k, c, W), hex(k)
        assert sum(dj << o for dj, o in zip(d, offs)) == k, hex(k)
        assert all(-sh.half <= dj < sh.half for dj in d[:-1]), hex(k)
        assert 0 <= d[-1] <= sh.top, hex(k)
        tops.add(d[-1])
    assert sh.top in tops   # r - 1 reaches it
