"""The lazy mixed addition xyzz_madd_lazy(acc, q, neg) (csrc/ec.hpp, csrc/ed25519.hpp) on RAW accumulator images AT the
bounds its comment states, shared by the host build (test_field_raw_cpu.py) and the device (test_gpu_raw_hooks.py).

Weierstrass curves: the accumulator of a known multiple m G is (X, Y, ZZ, ZZZ) = (x z^2, y z^3, z^2, z^3) for several z,
in Montgomery form, in EVERY representation the invariant allows: X + k p for k = 0..5 (X < 6p), Y + j p for j = 0, 1
(Y <= 2p), ZZ and ZZZ canonical (< 1.1p).  q is a canonical affine point: the same point and its negative with both signs
(the doubling, and the cancellation that fe_is_zero_mod<5> must see through the unreduced difference), a generic point,
infinity; and the accumulator itself at infinity, with ZZ spelt 0 and p.
edwards25519: extended coordinates (X, Y, Z, T) = (x z, y z, z, x y z), canonical (its comment: below 1.01 p), the
formula is complete; the same choices of q.

The affine result is compared with pyref's group law, and the output must keep the invariants: normalised limbs,
X < 6p, Y <= 2p, ZZ, ZZZ < 1.1p and ZZ^3 == ZZZ^2 (edwards25519: every coordinate below 1.01 p and X Y == Z T)."""

import functools
import random
from collections import namedtuple

import numpy as np

import pyref as P
from field_cases import FIELDS, LIMB_MASK, limb_array, values

MaddCases = namedtuple("MaddCases", "acc q neg want")   # (n, 4, NL), (n, 2, NL), (n,) uint32; want: affine points / None

CURVES = {"bls12_381": "bls12_381_fp", "secp256k1": "secp256k1_fp", "ed25519": "ed25519_fp"}


def _group(curve):
    return P.EdwardsGroup(P.CURVES[curve]) if curve == "ed25519" else P.WeierstrassGroup(P.CURVES[curve])


@functools.lru_cache(maxsize=None)
def cases(curve):
    f = FIELDS[CURVES[curve]]
    p, R = f.p, f.R
    G = _group(curve)
    g = G.base()
    ed = curve == "ed25519"
    rng = random.Random("madd lazy " + curve)
    mont = lambda v: v * R % p
    zs = [1, 2, p - 1, rng.randrange(2, p), rng.randrange(2, p)]
    accs, qs, negs, want = [], [], [], []

    def q_image(Q):
        if Q is None:
            return (0, mont(1)) if ed else (0, 0)
        return (mont(Q[0]), mont(Q[1]))

    def emit(acc, A, Q, neg):
        accs.append(acc)
        qs.append(q_image(Q))
        negs.append(neg)
        want.append(G.add(A, G.neg(Q) if neg else Q))

    def images(A, z):
        """every raw image of the accumulator that holds the affine point A with the given z"""
        x, y = A
        if ed:
            return [(mont(x * z), mont(y * z), mont(z), mont(x * y * z))]
        X, Y, ZZ, ZZZ = mont(x * z * z), mont(y * z * z * z), mont(z * z), mont(z * z * z)
        return [(X + k * p, Y + j * p, ZZ, ZZZ) for k in range(6) for j in range(2)]

    other = G.mul(g, 0x1234567)
    ms = [1, 2, 7, 0xABCDEF, G.r - 3]
    if ed:   # one image per accumulator: more multiples and more z instead, so that the cases fill more than one block
        ms += [3, 5, 0x10001, G.r - 1, G.r - 2]
        zs += [3, p - 2] + [rng.randrange(2, p) for _ in range(3)]
    for m, z in zip(ms, zs):
        A = G.mul(g, m)
        for acc in images(A, z):
            for Q in (A, G.neg(A)):          # doubling and cancellation, reached through either sign
                for neg in (0, 1):
                    emit(acc, A, Q, neg)
            emit(acc, A, other, rng.randrange(2))
            emit(acc, A, G.mul(g, rng.randrange(1, G.r)), rng.randrange(2))
        emit(images(A, z)[-1], A, None, 0)   # q at infinity: the accumulator stays as it is
        emit(images(A, z)[0], A, None, 1)
    # the accumulator at infinity
    if ed:
        infs = [(0, mont(1), mont(1), 0), (0, mont(5), mont(5), 0), (p, mont(5), mont(5), 0)]
    else:
        infs = [(mont(1), mont(1), 0, 0), (mont(1), mont(1), p, 0), (3, 4, 0, 5)]
    for acc in infs:
        for Q, neg in ((g, 0), (g, 1), (other, 1), (None, 0), (None, 1)):
            emit(acc, None, Q, neg)
    n = len(accs)
    acc = limb_array([v for a in accs for v in a], f.NL).reshape(n, 4, f.NL)
    q = limb_array([v for a in qs for v in a], f.NL).reshape(n, 2, f.NL)
    return MaddCases(acc, q, np.array(negs, dtype=np.uint32), want)


def check(curve, out):
    """out (n, 4, NL) uint32: the accumulators after xyzz_madd_lazy"""
    f = FIELDS[CURVES[curve]]
    p, R = f.p, f.R
    c = cases(curve)
    n = len(c.want)
    assert out.shape == (n, 4, f.NL) and out.dtype == np.uint32
    assert int(out.max()) <= LIMB_MASK, "limbs not normalised"
    Rinv = pow(R, -1, p)
    v = [values(out[:, t, :]) for t in range(4)]
    kinds = {"inf": 0, "point": 0}
    for i in range(n):
        raw = [v[t][i] for t in range(4)]
        a, b, c2, d = (x * Rinv % p for x in raw)
        where = "%s #%d neg=%d" % (curve, i, int(c.neg[i]))
        if curve == "ed25519":
            # below 1.01 p: products of operands with alpha beta <= 14 against R / p = 2^15
            assert all(100 * x < 101 * p for x in raw), where
            assert c2 != 0 and (a * b - c2 * d) % p == 0, where
            zi = pow(c2, -1, p)
            got = (a * zi % p, b * zi % p)
            got = None if got == (0, 1) else got
        else:
            X, Y, ZZ, ZZZ = raw
            assert X < 6 * p and Y <= 2 * p and 10 * ZZ < 11 * p and 10 * ZZZ < 11 * p, where
            if c2 == 0:
                got = None
            else:
                assert (pow(c2, 3, p) - d * d) % p == 0, where
                got = (a * pow(c2, -1, p) % p, b * pow(d, -1, p) % p)
        assert got == c.want[i], where
        kinds["inf" if got is None else "point"] += 1
    assert kinds["inf"] >= 10 and kinds["point"] >= 30
    assert n > 64   # more than one block of the device hook
