"""The scalar and half lists of the GLV tests, shared by the host builds (test_fixed_glv_cpu.py, test_host_arith_cpu.py)
and the device (test_gpu_glv.py): edges of the BLS12-381 split k = k1 + k2 z^2 and of its balanced form, of the signed
secp256k1 split, and of the digit recoding of a window layout."""

import random

import pyref as P

Z = 0xd201000000010000
Z2 = Z * Z
R = P.BLS12_381["r"]
HALF_MAX = Z2 // 2 + 1          # the stated bound on both magnitudes of the balanced split
SECP_N = P.SECP256K1["r"]
SECP_LAMBDA = 0x5363ad4cc05c30e0a5261c028812645a122e22ea20816678df02967c1b23bd72


def edges():
    """the scalars of the issue's list: 0, 1, r-1, the middle of the range, around z^2 and z^2/2, multiples of z^2, and the
    scalars that give the largest k1 and the largest k2"""
    ks = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, (R - 1) // 2 - 1, (R + 1) // 2 + 1,
          Z2 - 1, Z2, Z2 + 1, Z2 // 2, Z2 // 2 + 1, Z2 // 2 - 1, R - Z2, R - Z2 // 2, R - Z2 // 2 - 1]
    ks += [j * Z2 for j in (2, 3, 5, Z2 // 2 - 1, Z2 // 2, (R - 1) // (2 * Z2))]
    ks += [R - j * Z2 for j in (1, 2, 3, 7)]
    q_max = ((R - 1) // 2) // Z2                      # largest quotient of a scalar in the lower half of the range
    ks += [q_max * Z2 + d for d in (0, 1, Z2 // 2, Z2 // 2 + 1, ((R - 1) // 2) % Z2)]   # largest k2 (k1 folds upwards)
    ks += [j * Z2 + Z2 // 2 for j in (0, 1, 12345)]   # largest k1
    ks += [R - k for k in ks[-8:] if k]
    return [k % R for k in ks]


def bls_split_scalars():
    """glv_split: edges around z^2 and 2^128, random scalars, random multiples of z^2 plus 0, 1, z^2 - 1"""
    r, z2 = R, Z2
    rng = random.Random(11)
    ks = [0, 1, z2 - 1, z2, z2 + 1, 2 * z2 - 1, 2 * z2, r - 1, r - 2, (r // z2) * z2, (r // z2) * z2 - 1, (1 << 128) - 1, 1 << 128,
          (1 << 255) - 1 if (1 << 255) - 1 < r else r - 3]
    ks += [rng.randrange(r) for _ in range(3000)]
    ks += [rng.randrange(1 << 128) * z2 + d for d in (0, 1, z2 - 1) for _ in range(200) if True]
    return [k for k in ks if k < r]


def secp_split_scalars():
    """glv_split_signed on secp256k1: random scalars and the edges (0, 1, n - 1, lambda, n - lambda, the middle of the
    range, values that make either half negative)"""
    n, lam = SECP_N, SECP_LAMBDA
    rng = random.Random(12)
    ks = [0, 1, 2, n - 1, n - 2, lam, n - lam, lam + 1, lam - 1, (n - 1) // 2, (n + 1) // 2, (1 << 128) - 1, 1 << 128, (1 << 255),
          (1 << 256) - 1 - ((1 << 256) - n) - 5]
    ks += [rng.randrange(n) for _ in range(4000)]
    ks += [(a + b * lam) % n for a in (1, -1, (1 << 127) - 1, -(1 << 127) + 1) for b in (1, -1, (1 << 127) - 1, -(1 << 127) + 1)]
    return [k % n for k in ks]


RECODE_WINDOW_BITS = [10, 13, 16, 17]


def recode_halves(c, wins):
    """halves for the layout at window_bits c; wins: (width, offset, first entry) per window, the top window last"""
    offs = [o for _, o, _ in wins]
    rng = random.Random(22 + c)
    hs = [0, 1, 2, HALF_MAX, HALF_MAX - 1, Z2 // 2, Z2 // 4] + [1 << o for o in offs] + [(1 << o) - 1 for o in offs[1:]]
    hs += [(1 << (o + w - 1)) for w, o, _ in wins[:-1]] + [(1 << (o + w - 1)) - 1 for w, o, _ in wins[:-1]]
    hs += [rng.randrange(HALF_MAX + 1) for _ in range(5000)]
    return hs
