"""The cases and the integer reference of the raw-limb field tests, shared by the host build (test_field_raw_cpu.py) and
the device (test_gpu_field_raw.py): both run csrc/field_raw_ops.hpp, which takes operands as RAW 30-bit limb images --
no conversion on the way in or out -- so the multiplier and the unreduced sums see what the hot kernels feed them:
all-ones limbs, values up to 8 p, sums that were never reduced.

An operand is a Python integer v < K p written as NL limbs, v = sum l[i] 2^(30 i), every limb below 2^30; K is the
multiple of p the operation's comment in csrc/field.hpp allows (8 where it says "<= 8 p").  Per operand bound the values
are
  * limb patterns: every limb below the top all-ones with the largest top limb that keeps the value below k p
    (k = 1, 2, 8), and with the top limb zero; alternating all-ones / zero limbs in both phases; one limb all-ones and the rest zero, for each
    position; limb 0 = 1.  A pattern that reaches the bound gets the largest top limb that stays below it.
  * value edges: 0, 1, p - 1, p, p + 1, 2p - 1, 2p and k p - 1, k p, k p + 1 for every k up to the bound.
  * 1000 random values below the bound.
Binary operations take the full cross product of the edge lists plus random pairs; fe_mul_add takes quadruples of the
edge lists (all four equal, (a, b, a, b) over the cross product, random draws) plus random ones.

The reference is Python integers: R = 2^(30 NL);
  multiplicative      limbs normalised, out R == a b (+ c d) (mod p), out R <= a b (+ c d) + p R  (field.hpp, fe_mont_reduce)
  unreduced (nr)      exact integer equality, e.g. a - b + K p
  fe_add, fe_sub ..   congruent and in [0, 2p)
  predicates          the integer truth value
  inverses            pow(x, -1, p) in the operation's output form, 0 -> 0
"""

import functools
import itertools
import random
from collections import namedtuple

import numpy as np

import pyref as P

LIMB_BITS = 30
LIMB_MASK = (1 << LIMB_BITS) - 1
N_RANDOM = 1000

Field = namedtuple("Field", "name curve cid idx p NL N R")


def _field(name, curve, cid, idx, p):
    NL = 13 if p.bit_length() > 256 else 9
    return Field(name, curve, cid, idx, p, NL, 12 if NL == 13 else 8, 1 << (LIMB_BITS * NL))


FIELDS = {f.name: f for f in (
    _field("bls12_381_fp", "bls12_381", 0, 0, P.BLS12_381["p"]), _field("bls12_381_fr", "bls12_381", 0, 1, P.BLS12_381["r"]),
    _field("secp256k1_fp", "secp256k1", 1, 0, P.SECP256K1["p"]), _field("secp256k1_fr", "secp256k1", 1, 1, P.SECP256K1["r"]),
    _field("ed25519_fp", "ed25519", 2, 0, P.ED25519["p"]), _field("ed25519_fr", "ed25519", 2, 1, P.ED25519["r"]))}

# the RawOp codes of csrc/field_raw_ops.hpp
OPS = ["mul", "mul_io", "sqr", "sqr_io", "mul_add", "add", "sub", "neg", "dbl", "add_nr", "sub_nr1", "sub_nr2", "sub_nr4",
       "sub_nr6", "csub_nr4_pos", "csub_nr4_neg", "add_dbl_nr", "is_zero", "is_zero_mod5", "eq", "cond_sub_p", "to_canonical",
       "store_load", "from_u32", "from_i32", "inv", "inv_plain", "inv_fermat", "pow_u64"]
OP_CODE = {name: i for i, name in enumerate(OPS)}

Case = namedtuple("Case", "op code A B C D")   # A..D: lists of integers, one per element (B..D zeros where unused)


def limbs(v, NL):
    assert 0 <= v < 1 << (LIMB_BITS * NL)
    return tuple((v >> (LIMB_BITS * i)) & LIMB_MASK for i in range(NL))


def limb_array(vals, NL):
    cache = {}
    rows = []
    for v in vals:
        r = cache.get(v)
        if r is None:
            r = cache[v] = limbs(v, NL)
        rows.append(r)
    return np.array(rows, dtype=np.uint32).reshape(len(vals), NL)


def values(arr, bits=LIMB_BITS):
    """rows of little-endian `bits`-bit digits -> list of Python integers"""
    acc = np.zeros(arr.shape[0], dtype=object)
    for i in range(arr.shape[1]):
        acc = acc + (arr[:, i].astype(object) << (bits * i))
    return [int(x) for x in acc]


def edge_values(f, K, inclusive=False):
    """the limb patterns and value edges below K p (up to K p itself when `inclusive`), in a fixed order"""
    p, NL = f.p, f.NL
    limit = K * p + (1 if inclusive else 0)
    shift = LIMB_BITS * (NL - 1)
    low = (1 << shift) - 1

    def clamp(v):   # the largest top limb that keeps the value below the limit (p > 2^shift: there always is one)
        return v if v < limit else (v & low) | (((limit - 1 - (v & low)) >> shift) << shift)

    pats = [low | (((k * p - 1 - low) >> shift) << shift) for k in (1, 2, 8) if k <= K]
    pats += [low]   # ... and with the top limb zero
    pats += [sum(LIMB_MASK << (LIMB_BITS * i) for i in range(ph, NL, 2)) for ph in (0, 1)]
    pats += [LIMB_MASK << (LIMB_BITS * i) for i in range(NL)]
    pats += [1]
    edges = [0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p]
    for k in range(1, K + 1):
        edges += [k * p - 1, k * p, k * p + 1]
    out = []
    for v in [clamp(v) for v in pats] + [v for v in edges if v < limit]:
        assert v < limit and v < f.R
        if v not in out:
            out.append(v)
    return out


def _pool(f, K, rng, inclusive=False):
    return [rng.randrange(K * f.p + (1 if inclusive else 0)) for _ in range(N_RANDOM)]


def _pairs(f, Ka, Kb, rng, inclusive=False, keep=None):
    ea, eb = edge_values(f, Ka, inclusive), edge_values(f, Kb, inclusive)
    pa, pb = _pool(f, Ka, rng, inclusive), _pool(f, Kb, rng, inclusive)
    pairs = list(itertools.product(ea, eb)) + list(zip(pa, pb))
    pairs += [(rng.choice(ea), b) for b in pb[:200]] + [(a, rng.choice(eb)) for a in pa[:200]]
    if keep:
        n_all = len(pairs)
        pairs = [ab for ab in pairs if keep(*ab)]
        assert len(pairs) > n_all // 8   # the filter leaves a real share of the edges and of the random pairs
    return [a for a, _ in pairs], [b for _, b in pairs]


def _inverse_inputs(f, rng):
    p = f.p
    xs = [0, 1, p - 1, (p - 1) // 2, (p + 1) // 2]
    for k in range(p.bit_length()):
        if (1 << k) < p:
            xs += [1 << k, p - (1 << k)]
    xs += [v for v in edge_values(f, 1)]
    seen, out = set(), []
    for x in xs:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out + [rng.randrange(p) for _ in range(N_RANDOM)]


@functools.lru_cache(maxsize=None)
def cases(fname):
    """every Case of one field, built once per process"""
    f = FIELDS[fname]
    p = f.p
    rng = random.Random("raw limbs " + fname)
    out = []

    def add(op, A, B=None, C=None, D=None):
        z = [0] * len(A)
        out.append(Case(op, OP_CODE[op], list(A), list(B or z), list(C or z), list(D or z)))

    def unary(K):
        return edge_values(f, K) + _pool(f, K, rng)

    # the multiplier: operands below 8 p ("<= 8 p" of the lazy formulas)
    for op in ("mul", "mul_io"):
        add(op, *_pairs(f, 8, 8, rng))
    for op in ("sqr", "sqr_io"):
        add(op, unary(8))
    e8, pool8 = edge_values(f, 8), _pool(f, 8, rng)
    quads = [(e, e, e, e) for e in e8]
    quads += [(a, b, a, b) for a, b in itertools.product(e8, e8)]
    quads += [tuple(rng.choice(e8) for _ in range(4)) for _ in range(N_RANDOM)]
    quads += [tuple(rng.choice(pool8) for _ in range(4)) for _ in range(N_RANDOM)]
    quads += [tuple(rng.choice(e8 if rng.random() < 0.5 else pool8) for _ in range(4)) for _ in range(N_RANDOM)]
    add("mul_add", *([q[i] for q in quads] for i in range(4)))
    # reduced sums: operands in [0, 2p)
    for op in ("add", "sub", "eq"):
        add(op, *_pairs(f, 2, 2, rng))
    for op in ("neg", "dbl", "is_zero", "cond_sub_p", "store_load"):
        add(op, unary(2))
    # unreduced sums: a below 8 p; the subtrahend at most K p
    add("add_nr", *_pairs(f, 8, 8, rng))
    add("add_dbl_nr", *_pairs(f, 8, 8, rng))
    for K in (1, 2, 4, 6):
        A, B = _pairs(f, 8, K, rng)
        ib = edge_values(f, K, inclusive=True)   # b = K p itself is allowed
        add("sub_nr%d" % K, A + [rng.choice(A) for _ in ib], B + ib)
    for op in ("csub_nr4_pos", "csub_nr4_neg"):   # the caller guarantees a + b <= 4 p
        add(op, *_pairs(f, 4, 4, rng, inclusive=True, keep=lambda a, b: a + b <= 4 * p))
    add("is_zero_mod5", edge_values(f, 6) + _pool(f, 6, rng) + [k * p for k in range(6) for _ in range(4)])
    add("to_canonical", unary(8))
    # scalars in words: a[0] is the argument
    u32 = [0, 1, 2, LIMB_MASK, LIMB_MASK + 1, LIMB_MASK + 2, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 2, (1 << 32) - 1]
    u32 += [rng.randrange(1 << 32) for _ in range(N_RANDOM)]
    add("from_u32", u32)
    add("from_i32", u32)
    # inverses: Montgomery-form operand in [0, 2p) for fe_inv (every residue also as x + p), plain residue below p for
    # fe_inv_plain
    inv = _inverse_inputs(f, rng)
    add("inv", inv + [x + p for x in inv])
    add("inv_plain", inv)
    add("inv_fermat", inv + [x + p for x in inv[:64]])
    # powers: exponent in b[0] | b[1] << 32
    exps = [0, 1, 2, 3, 5, (1 << 30) - 1, 1 << 30, (1 << 32) - 1, 1 << 32, (1 << 63) + 1, (1 << 64) - 1]
    base = edge_values(f, 2)
    A = [a for a in base for _ in exps] + _pool(f, 2, rng)
    B = [e for _ in base for e in exps] + [rng.randrange(1 << 64) >> rng.randrange(64) for _ in range(N_RANDOM)]
    add("pow_u64", A, B)
    assert sorted(c.op for c in out) == sorted(OPS)
    return out


def operand_arrays(f, case):
    """the four operand arrays (n, NL) uint32 of a case; scalar arguments go into the first words as they are"""
    if case.op in ("from_u32", "from_i32"):
        a = np.zeros((len(case.A), f.NL), dtype=np.uint32)
        a[:, 0] = np.array(case.A, dtype=np.uint64).astype(np.uint32)
    else:
        a = limb_array(case.A, f.NL)
    if case.op == "pow_u64":
        b = np.zeros((len(case.B), f.NL), dtype=np.uint32)
        e = np.array(case.B, dtype=np.uint64)
        b[:, 0] = (e & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        b[:, 1] = (e >> np.uint64(32)).astype(np.uint32)
    else:
        b = limb_array(case.B, f.NL)
    return a, b, limb_array(case.C, f.NL), limb_array(case.D, f.NL)


def check(f, case, out):
    """asserts that `out` (n, 2 NL) uint32, what fe_raw_op wrote for the case, is what the integers say"""
    p, NL, N, R = f.p, f.NL, f.N, f.R
    op, n = case.op, len(case.A)
    assert out.shape == (n, 2 * NL) and out.dtype == np.uint32
    A, B, C, D = case.A, case.B, case.C, case.D
    where = lambda i: "%s %s #%d a=%x b=%x c=%x d=%x" % (f.name, op, i, A[i], B[i], C[i], D[i])
    lo, hi = out[:, :NL], out[:, NL:]
    if op in ("is_zero", "is_zero_mod5", "eq"):
        assert not out[:, 1:].any()
        want = [(a - b) % p == 0 for a, b in zip(A, B)]   # b = 0 for the unary predicates
        assert want.count(True) >= 2 and want.count(False) >= 2, "the cases must hold both answers"
        for i in range(n):
            assert int(out[i, 0]) == int(want[i]), where(i)
        return
    if op == "to_canonical":
        assert not out[:, N:].any()
        got = values(out[:, :N], 32)
        Rinv = pow(R, -1, p)
        for i in range(n):
            assert got[i] == A[i] * Rinv % p, where(i)
        return
    assert int(lo.max()) <= LIMB_MASK, "%s %s: limbs not normalised" % (f.name, op)
    O = values(lo)
    if op in ("mul_io", "sqr_io"):
        assert np.array_equal(hi, limb_array(A, NL)), "%s %s: the operand did not come back unchanged" % (f.name, op)
    elif op == "store_load":
        assert not out[:, NL + N:].any()
        W = values(out[:, NL:NL + N], 32)
        for i in range(n):
            assert W[i] == A[i] % p, where(i)
    else:
        assert not hi.any()

    if op in ("mul", "mul_io", "sqr", "sqr_io", "mul_add"):
        for i in range(n):
            a, b = A[i], (A[i] if op in ("sqr", "sqr_io") else B[i])
            T = a * b + (C[i] * D[i] if op == "mul_add" else 0)
            assert (O[i] * R - T) % p == 0, where(i)
            assert O[i] * R <= T + p * R, where(i)
    elif op in ("add", "sub", "neg", "dbl"):
        for i in range(n):
            want = {"add": A[i] + B[i], "sub": A[i] - B[i], "neg": -A[i], "dbl": 2 * A[i]}[op]
            assert (O[i] - want) % p == 0 and 0 <= O[i] < 2 * p, where(i)
    elif op == "add_nr":
        for i in range(n):
            assert O[i] == A[i] + B[i], where(i)
    elif op == "add_dbl_nr":
        for i in range(n):
            assert O[i] == A[i] + 2 * B[i], where(i)
    elif op.startswith("sub_nr"):
        K = int(op[6:])
        for i in range(n):
            assert B[i] <= K * p and O[i] == A[i] - B[i] + K * p, where(i)
    elif op.startswith("csub_nr4"):
        s = -1 if op.endswith("neg") else 1
        for i in range(n):
            assert A[i] + B[i] <= 4 * p and O[i] == s * A[i] - B[i] + 4 * p, where(i)
    elif op == "cond_sub_p":
        for i in range(n):
            assert O[i] == (A[i] - p if A[i] >= p else A[i]), where(i)
    elif op == "store_load":
        for i in range(n):
            assert O[i] == A[i] % p, where(i)
    elif op in ("from_u32", "from_i32"):
        for i in range(n):
            x = A[i] - (1 << 32) if op == "from_i32" and A[i] >> 31 else A[i]
            assert (O[i] - x * R) % p == 0 and O[i] < 2 * p, where(i)
    elif op == "inv_plain":
        for i in range(n):
            assert O[i] == (pow(A[i], -1, p) if A[i] else 0), where(i)
    elif op in ("inv", "inv_fermat"):
        # operand x R, result x^-1 R: out == a^-1 R^2 (mod p); 0 -> 0
        R2 = R * R % p
        for i in range(n):
            a = A[i] % p
            assert O[i] < 2 * p, where(i)
            if a == 0:
                assert O[i] % p == 0 and (O[i] == 0 or (op == "inv_fermat" and A[i] != 0)), where(i)
            else:
                assert O[i] % p == pow(a, -1, p) * R2 % p, where(i)
    elif op == "pow_u64":
        Rinv = pow(R, -1, p)
        for i in range(n):
            assert O[i] % p == pow(A[i] * Rinv % p, B[i], p) * R % p and O[i] < 2 * p, where(i)
    else:
        raise AssertionError("no reference for " + op)


def run_and_check(fname, run):
    """run(field, op code, a, b, c, d) -> (n, 2 NL) uint32, for every case of the field"""
    f = FIELDS[fname]
    seen = []
    for case in cases(fname):
        a, b, c, d = operand_arrays(f, case)
        check(f, case, run(f, case.code, a, b, c, d))
        seen.append(case.op)
    assert sorted(seen) == sorted(OPS)


# the quadruple that overflowed the one plain-product accumulator of fe_mul_add's middle columns on the 13-limb field:
# limbs 0..11 all-ones, limb 12 zero -- 2^360 - 1, normalised and below p
OVERFLOW_PROBE = (1 << 360) - 1
