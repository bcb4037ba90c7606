"""Shared case builder of the scalar-stage tests (CPU: test_scalar_cases_cpu.py, GPU: test_gpu_verifier_scalars.py): full
challenge sets [y, z, e, e_1..e_k] with proof scalars [r', s', delta'], and the N = 2 mn + 2 k + m + 5 MulVec scalars the
DEFINITION gives them.  Nothing here imports the product: the cases are built with oracle/pyref.py and big integers alone.

Two restatements of each scalar list:
  range_scalars / seam_scalars                 pyref's verify_mulvec over the shadow group (dummy points), with the
                                               Transcript literals set to the row's challenges for the call;
  range_scalars_direct / seam_scalars_direct   the closed forms written out index by index -- the comment above
                                               k_vs_prepare (csrc/kernels.hpp) with range/mod.rs:189-238 (m = 1) and :405-477
                                               (m > 1), and wip.rs:238-320 for the seam -- sharing nothing with pyref but pow.
They differ in ONE place: the direct forms use inv0(x) = x^-1, and 0 for x = 0 -- what the kernels state ("zero entries are
skipped, their inverse stays 0") -- where pyref's pow(0, -1, r) raises.  Negative powers of y are inv0(y)^j and allinv is the
product of the inv0(e_t).  For a challenge that is 0 mod r the direct form IS the definition.

Every input is a 256-bit word pattern and is defined as its residue mod r (fe_from_canonical's contract, csrc/field.hpp):
both restatements reduce first.  lifts() lists the patterns >= r that stand for a residue.

MulVec order: m > 1  [1, e^-1, e^-2, g_exp, h_exp, e_t^2 (k), e_t^-2 (k), G_exp (mn), H_exp (mn), V_exp (m)]
              m = 1 and the seam  [1, e, e^2, g_exp, h_exp, e_t^2 e^2 (k), e_t^-2 e^2 (k), G_exp, H_exp, V_exp]
"""

import random

import numpy as np

import pyref as P

CURVES = ("bls12_381", "secp256k1", "ed25519")
TOP = (1 << 256) - 1


def order(curve):
    return P.CURVES[curve]["r"]


def log2(mn):
    k = mn.bit_length() - 1
    assert mn == 1 << k
    return k


def n_scalars(n, m):
    return 2 * n * m + 2 * log2(n * m) + m + 5


def inv0(x, r):
    x %= r
    return pow(x, -1, r) if x else 0


# ---- words >= r ----------------------------------------------------------------------------------------------------
def lifts(curve, x):
    """every 256-bit pattern x + j r, j >= 1, of the residue x (none on secp256k1 unless x < 2^256 - r)"""
    r = order(curve)
    x %= r
    return list(range(x + r, 1 << 256, r))


def liftable(curve):
    """residues below this bound have at least one lift on the curve"""
    return min(order(curve), (1 << 256) - order(curve))


def lift(curve, x):
    """the largest pattern of the residue x (bls12_381: x + r or x + 2 r, edwards25519: x + 15 r, ...)"""
    return lifts(curve, x)[-1]


# ---- through pyref -------------------------------------------------------------------------------------------------
class _Literals:
    """pyref.Transcript's literals set to one row's challenges for the duration of a call"""

    NAMES = ("Y_SINGLE", "Z_SINGLE", "Y_MULTI", "Z_MULTI", "E_FINAL", "E_ROUND")

    def __init__(self, y, z, e, e_rounds):
        self.new = (y, z, y, z, e, list(e_rounds))

    def __enter__(self):
        T = P.Transcript
        assert T.fs is None and T.cached is None
        self.saved = tuple(getattr(T, a) for a in self.NAMES)
        for a, v in zip(self.NAMES, self.new):
            setattr(T, a, v)

    def __exit__(self, *exc):
        for a, v in zip(self.NAMES, self.saved):
            setattr(P.Transcript, a, v)


_shadow_keys = {}


def _shadow_pk(r, length):
    if (r, length) not in _shadow_keys:
        _shadow_keys[(r, length)] = P.PublicKey(P.ShadowGroup(r), length)
    return _shadow_keys[(r, length)]


def range_scalars(curve, n, m, y, z, e, e_rounds, s3):
    """RangeProof.verify_mulvec(...).scalars over the shadow group; raises (pow) on a challenge pyref has to invert that is
    0 mod r"""
    r = order(curve)
    k = log2(n * m)
    assert len(e_rounds) == k and len(s3) == 3
    wip = P.WeightedInnerProductProof([0] * k, [0] * k, 0, 0, s3[0] % r, s3[1] % r, s3[2] % r)
    with _Literals(y % r, z % r, e % r, [x % r for x in e_rounds]):
        mv = P.RangeProof(0, wip).verify_mulvec(_shadow_pk(r, n * m), n, [0] * m)
    assert len(mv.scalars) == n_scalars(n, m)
    return mv.scalars


def seam_scalars(curve, length, y, stm, e, e_rounds, s3):
    """WeightedInnerProductProof.verify_mulvec(...).scalars for the statement block stm = [Gc (len), Hc (len), gc, Vc (nv)]"""
    r = order(curve)
    k = log2(length)
    nv = len(stm) - 2 * length - 1
    assert len(e_rounds) == k and nv >= 0
    stm = [x % r for x in stm]
    wip = P.WeightedInnerProductProof([0] * k, [0] * k, 0, 0, s3[0] % r, s3[1] % r, s3[2] % r)
    with _Literals(0, 0, e % r, [x % r for x in e_rounds]):
        mv = wip.verify_mulvec(_shadow_pk(r, length), P.Fr(r).exp_iter_type2(y % r, length), stm[:length],
                               stm[length:2 * length], stm[2 * length], stm[2 * length + 1:], 0, [0] * nv)
    assert len(mv.scalars) == 2 * length + 2 * k + 5 + nv
    return mv.scalars


# ---- written out ---------------------------------------------------------------------------------------------------
def _s_vec(r, k, e_rounds):
    """s[i] = prod_t inv0(e_t) * prod_{bit b of i set} e_{k-1-b}^2    (wip.rs:372-380 unrolled)"""
    allinv = 1
    for x in e_rounds:
        allinv = allinv * inv0(x, r) % r
    s = []
    for i in range(1 << k):
        v = allinv
        for b in range(k):
            if (i >> b) & 1:
                v = v * e_rounds[k - 1 - b] % r * e_rounds[k - 1 - b] % r
        s.append(v)
    return s


def range_scalars_direct(curve, n, m, y, z, e, e_rounds, s3):
    r = order(curve)
    mn = n * m
    k = log2(mn)
    assert len(e_rounds) == k and len(s3) == 3
    y, z, e = y % r, z % r, e % r
    er = [x % r for x in e_rounds]
    rp, sp, dp = (x % r for x in s3)
    yinv = inv0(y, r)
    s = _s_vec(r, k, er)
    zsq = z * z % r
    sum_y = 0                                   # y + y^2 + .. + y^mn
    for i in range(1, mn + 1):
        sum_y = (sum_y + pow(y, i, r)) % r
    y_top = pow(y, mn + 1, r)
    two_n1 = (pow(2, n, r) - 1) % r             # 1 + 2 + .. + 2^(n-1)
    out = [1]
    if m == 1:
        esq = e * e % r
        out += [e, esq]
        gc = (sum_y * (z - zsq) - two_n1 * y_top % r * z) % r
        out.append((-rp * y % r * sp + gc * esq) % r)
        out.append(-dp % r)
        out += [x * x % r * esq % r for x in er]
        out += [inv0(x, r) ** 2 % r * esq % r for x in er]
        for i in range(n):
            out.append((-z * esq - s[i] * pow(yinv, i + 1, r) % r * rp % r * e % r * y) % r)
        for i in range(n):
            out.append(((pow(2, i, r) * pow(y, n - i, r) + z) * esq - s[n - 1 - i] * sp % r * e) % r)
        out.append(y_top * esq % r)
        return out
    einv = inv0(e, r)
    einv2 = einv * einv % r
    out += [einv, einv2]
    sum_z = 0                                   # z^2 + z^4 + .. + z^(2m)
    for j in range(1, m + 1):
        sum_z = (sum_z + pow(zsq, j, r)) % r
    gc = (sum_y * (z - zsq) - y_top * z % r * two_n1 % r * sum_z) % r
    out.append((-rp * sp % r * y % r * einv2 + gc) % r)
    out.append(-dp * einv2 % r)
    out += [x * x % r for x in er]
    out += [inv0(x, r) ** 2 % r for x in er]
    for i in range(mn):
        out.append((-z - s[i] * pow(yinv, i + 1, r) % r * rp % r * einv % r * y) % r)
    for i in range(mn):
        d = pow(2, i % n, r) * pow(zsq, i // n + 1, r) % r
        out.append((d * pow(y, mn - i, r) + z - sp * einv % r * s[mn - 1 - i]) % r)
    out += [pow(zsq, j + 1, r) * y_top % r for j in range(m)]
    return out


def seam_scalars_direct(curve, length, y, stm, e, e_rounds, s3):
    r = order(curve)
    k = log2(length)
    assert len(e_rounds) == k and len(stm) >= 2 * length + 1
    y, e = y % r, e % r
    er = [x % r for x in e_rounds]
    stm = [x % r for x in stm]
    rp, sp, dp = (x % r for x in s3)
    yinv = inv0(y, r)
    s = _s_vec(r, k, er)
    esq = e * e % r
    out = [1, e, esq, (stm[2 * length] * esq - rp * y % r * sp) % r, -dp % r]
    out += [x * x % r * esq % r for x in er]
    out += [inv0(x, r) ** 2 % r * esq % r for x in er]
    for i in range(length):
        out.append((stm[i] * esq - s[i] * pow(yinv, i + 1, r) % r * rp % r * e % r * y) % r)
    for i in range(length):
        out.append((stm[length + i] * esq - s[length - 1 - i] * sp % r * e) % r)
    out += [v * esq % r for v in stm[2 * length + 1:]]
    return out


# ---- rows ----------------------------------------------------------------------------------------------------------
class Row:
    """one full challenge set as handed over (256-bit patterns: a value >= r stands for its residue)"""

    def __init__(self, name, y, z, e, e_rounds, s3):
        self.name, self.y, self.z, self.e, self.e_rounds, self.s3 = name, y, z, e, list(e_rounds), list(s3)

    def args(self):
        return self.y, self.z, self.e, self.e_rounds, self.s3

    def challenges(self):
        return [self.y, self.z, self.e] + self.e_rounds

    def residues(self, r):
        return Row(self.name, self.y % r, self.z % r, self.e % r, [x % r for x in self.e_rounds], [x % r for x in self.s3])

    def replace(self, **kw):
        d = dict(name=self.name, y=self.y, z=self.z, e=self.e, e_rounds=list(self.e_rounds), s3=list(self.s3))
        d.update(kw)
        return Row(**d)


def _wide(rng, r):
    """a full-width non-zero residue"""
    return rng.randrange(r >> 1, r)


def _distinct(rng, r, cnt):
    out = []
    while len(out) < cnt:
        x = _wide(rng, r)
        if x not in out:
            out.append(x)
    return out


def random_row(curve, k, rng, name="random"):
    r = order(curve)
    y, z, e = _distinct(rng, r, 3)
    return Row(name, y, z, e, _distinct(rng, r, k), [rng.randrange(r) for _ in range(3)])


def row_names(k):
    """the non-zero rows of a shape with k rounds"""
    return (["random"] + ["one_hot(%d)" % t for t in range(k)] +
            ["ones", "minus_ones", "y_half", "y_two", "z_zero", "z_one", "proof_scalars(0)", "proof_scalars(1)",
             "proof_scalars(2)", "lifted"])


def zero_row_names(k):
    names = ["zero_y", "zero_e", "zero_y_lifted", "zero_e_lifted"]
    for t in sorted({0, k - 1} if k else ()):
        names += ["zero_round(%d)" % t, "zero_round_lifted(%d)" % t]
    return names


def _arg(name):
    return int(name[name.index("(") + 1:-1])


def make_row(curve, k, name, rng):
    """the row `name`; everything a row does not pin is a distinct full-width value drawn from rng"""
    r = order(curve)
    base = random_row(curve, k, rng, name)
    if name == "random":
        return base
    if name.startswith("one_hot("):            # names the round whose index mapping is wrong
        t = _arg(name)
        return base.replace(e_rounds=[base.e_rounds[j] if j == t else 1 for j in range(k)])
    if name == "ones":
        return base.replace(y=1, z=1, e=1, e_rounds=[1] * k)
    if name == "minus_ones":
        return base.replace(y=r - 1, z=r - 1, e=r - 1, e_rounds=[r - 1] * k)
    if name == "y_half":                       # 2 y^-1 = 4: t_lo = 4^l; with y_two it is all ones
        return base.replace(y=pow(2, -1, r))
    if name == "y_two":
        return base.replace(y=2)
    if name == "z_zero":                       # legitimate: nothing inverts z
        return base.replace(z=0)
    if name == "z_one":                        # z - z^2 = 0
        return base.replace(z=1)
    if name.startswith("proof_scalars("):      # r', s', delta' from {0, 1, r - 1}, each value once in each place
        t = _arg(name)
        vals = [0, 1, r - 1]
        return base.replace(s3=[vals[(j + t) % 3] for j in range(3)])
    if name == "lifted":                       # y, e, one e_t and r' as words >= r; z as the all-ones word
        bound = liftable(curve)
        small = lambda: rng.randrange(bound >> 1, bound)
        y, e, rp = lift(curve, small()), lift(curve, small()), lift(curve, small())
        er = list(base.e_rounds)
        if k:
            er[k // 2] = lift(curve, small())
        return base.replace(y=y, z=TOP, e=e, e_rounds=er, s3=[rp] + base.s3[1:])
    if name in ("zero_y", "zero_y_lifted"):
        return base.replace(y=0 if name == "zero_y" else lift(curve, 0))
    if name in ("zero_e", "zero_e_lifted"):
        return base.replace(e=0 if name == "zero_e" else r)
    if name.startswith("zero_round"):
        t = _arg(name)
        er = list(base.e_rounds)
        er[t] = lift(curve, 0) if "lifted" in name else 0
        return base.replace(e_rounds=er)
    raise KeyError(name)


def zeroed(name):
    """which challenge a zero row zeroes: 'y', 'e' or a round index"""
    return "y" if "zero_y" in name else "e" if "zero_e" in name else _arg(name)


def healed(row, value):
    """the zero row with its zero replaced by `value`"""
    w = zeroed(row.name)
    if w == "y":
        return row.replace(name="healed", y=value)
    if w == "e":
        return row.replace(name="healed", e=value)
    er = list(row.e_rounds)
    er[w] = value
    return row.replace(name="healed", e_rounds=er)


def independent_outputs(n, m, what, seam=False):
    """indices of the MulVec scalars that do not depend on challenge `what` ('y', 'e' or round t), read off the closed
    forms: head [0..2], g_exp 3, h_exp 4, L 5.., R 5 + k.., G, H, V"""
    mn = n if seam else n * m           # the seam: n = its length, m = nv
    k = log2(mn)
    L, R = list(range(5, 5 + k)), list(range(5 + k, 5 + 2 * k))
    V = list(range(5 + 2 * k + 2 * mn, 5 + 2 * k + 2 * mn + m))
    if what == "y":        # y enters g_exp, every G_exp and (range) every H_exp and V_exp; the seam's H_exp, V_exp have none
        H = list(range(5 + 2 * k + mn, 5 + 2 * k + 2 * mn))
        return [0, 1, 2, 4] + L + R + (H + V if seam else [])
    if what == "e":
        if m == 1 or seam:  # e scales everything but the leading 1 and h_exp = -delta'
            return [0, 4]
        return [0] + L + R + V      # m > 1: e^-1 sits in the head, g_exp, h_exp, G_exp, H_exp
    t = what                # a round challenge: its own L, R and -- through s_vec -- every G_exp, H_exp
    return [0, 1, 2, 3, 4] + [i for i in L + R if i not in (5 + t, 5 + k + t)] + V


def rows(curve, n, m, count, seed, names=None):
    """`count` rows cycling through `names` (default: all non-zero rows of the shape); each pass draws fresh values"""
    k = log2(n * m)
    names = row_names(k) if names is None else list(names)
    rng = random.Random("%s %d %d %d" % (curve, n, m, seed))
    return [make_row(curve, k, names[i % len(names)], rng) for i in range(count)]


# ---- the seam's rows ---------------------------------------------------------------------------------------------------
class SeamRow:
    def __init__(self, name, y, stm, e, e_rounds, s3):
        self.name, self.y, self.stm, self.e, self.e_rounds, self.s3 = name, y, list(stm), e, list(e_rounds), list(s3)

    def args(self):
        return self.y, self.stm, self.e, self.e_rounds, self.s3

    def challenges(self):
        return [self.e] + self.e_rounds


def seam_row_names(k):
    return (["random"] + ["one_hot(%d)" % t for t in range(k)] + ["ones", "minus_ones", "lifted", "y_half", "zero_e"] +
            ["zero_round(%d)" % t for t in sorted({0, k - 1})])


def seam_rows(curve, length, nv, count, seed, names=None):
    """random statement, random y (y_half: 2^-1) and proof scalars; challenges [e, e_1..e_k] by the range rows' recipes"""
    r = order(curve)
    k = log2(length)
    names = seam_row_names(k) if names is None else list(names)
    rng = random.Random("seam %s %d %d %d" % (curve, length, nv, seed))
    out = []
    for i in range(count):
        name = names[i % len(names)]
        b = make_row(curve, k, name, rng)
        stm = [rng.randrange(r) for _ in range(2 * length + 1 + nv)]
        out.append(SeamRow(name, b.y, stm, b.e, b.e_rounds, b.s3))
    return out


# ---- wire ------------------------------------------------------------------------------------------------------------
def to_wire(xs):
    """ints < 2^256 -> (len, 4) uint64, little-endian words"""
    xs = list(xs)
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(len(xs), 4).copy()
