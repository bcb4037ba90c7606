"""Synthetic rows for mask recovery: proofs that no prover made.  A row names a curve, a shape (n, m), a challenge block
[y, z, e, e_1..e_k], a blinding source -- the 5 + 2k scalars themselves ("buffer") or a key and an index expanded with
oracle.blinding_from_key ("key") -- and chosen gammas.  Its delta' is built FORWARD, in the prover's direction
(delta_prime below; reference src/range/mod.rs:159-172, src/weighted_inner_product_proof.rs:171-227), so the expected
Gamma of a row is recover_cases.gamma_of(r, gammas, z): never recover_bigint (the inverse direction, which
tests/test_recover_rows_cpu.py holds against it) and never the library.

A ZERO row keeps the delta' of a non-zero row and sets one challenge to zero: an inversion is then undefined, the expected
result is Gamma = 0 with the flag up -- except z = 0 at m = 1, which the formula never reads: the mask is still gamma_0.

Shapes: make_shape takes n, m <= 64, so k = log2(n m) runs over 0..12; shapes(k) lists an m = 1 and an m > 1 shape wherever
both exist.  The GPU tests take the rows of the shapes their verifiers have."""

import hashlib
import random

import recover_cases as RC

CURVES = ("bls12_381", "secp256k1", "ed25519")
KS = tuple(range(13))
OWNER = hashlib.sha256(b"recover rows: the owning key").digest()
FOREIGN = [hashlib.sha256(b"recover rows: foreign key %d" % i).digest() for i in range(8)]
TOP_VALUES = 10      # r - 1, r - 2 and the eight limb-boundary values
SOURCES = ("buffer", "key")


def log2(x):
    assert x > 0 and not x & (x - 1)
    return x.bit_length() - 1


def shapes(k):
    """the shapes (n, m) with n m = 2^k that the suite runs: m = 1 where n = 2^k <= 64, m > 1 as a view of (1,64) or (64,64)"""
    out = []
    if k <= 6:
        out.append((1 << k, 1))
    if 1 <= k <= 6:
        out.append((1, 1 << k))
    if k >= 7:
        out.append((64, 1 << (k - 6)))
    return out


def top_values(r):
    """r - 1, r - 2 and, for j = 1..8, the largest value below r whose low 30 j bits are all ones: the limb boundaries of
    fe_from_canonical"""
    out = [r - 1, r - 2]
    for j in range(1, 9):
        low = (1 << (30 * j)) - 1
        v = (r >> (30 * j) << (30 * j)) | low
        if v >= r:
            v -= 1 << (30 * j)
        assert 0 < v < r and v & low == low
        out.append(v)
    assert len(out) == TOP_VALUES
    return out


def row_names(k, source):
    """every named row of a shape with log2(n m) = k.  top(i): enough rows that each of the ten top values occurs;
    blind_edges(i): the three rotations of 0, 1, r - 1 over the slots (a buffer's rows: a key expands to what it expands to)"""
    names = ["random", "zero(y)", "zero(z)", "zero(e)"] + ["zero(e_%d)" % t for t in range(k)] + ["minus_one", "one"]
    names += ["top(%d)" % i for i in range(-(-TOP_VALUES // (3 + k)))]
    if source == "buffer":
        names += ["blind_edges(%d)" % i for i in range(3)]
    return names + ["gamma_zero", "delta_edges(0)", "delta_edges(-1)"]


def is_zero_name(name):
    return name.startswith("zero(")


def zero_position(name, k):
    """the place in [y, z, e, e_1..e_k] that a zero row zeroes"""
    what = name[5:-1]
    return {"y": 0, "z": 1, "e": 2}[what] if what in ("y", "z", "e") else 3 + int(what[2:])


# ---- the prover's direction --------------------------------------------------------------------------------------------
def alpha_k(r, n, m, ch, blind, gammas):
    """alpha after the last round: alpha + y^(nm+1) S + sum_t (e_t^2 d_L[t] + e_t^-2 d_R[t]); S = gamma_0 for m = 1, else
    sum_j z^(2(j+1)) gamma_j.  Every round challenge must be invertible."""
    k = log2(n * m)
    y, z, et = ch[0], ch[1], ch[3:]
    s = sum(pow(z, 2 * (j + 1) if m > 1 else 0, r) * g for j, g in enumerate(gammas))
    a = blind[0] + pow(y, n * m + 1, r) * s
    for t in range(k):
        a += et[t] ** 2 * blind[5 + t] + pow(et[t], r - 3, r) * blind[5 + k + t]
    return a % r


def delta_prime(r, n, m, ch, blind, gammas):
    """delta' = eta + delta e + alpha_k e^2"""
    e = ch[2]
    return (blind[4] + blind[3] * e + alpha_k(r, n, m, ch, blind, gammas) * e * e) % r


def solve_gamma0(r, n, m, ch, blind, gammas, target):
    """gamma_0 such that delta_prime(.., [gamma_0] + gammas[1:]) == target: the forward recurrence is affine in gamma_0"""
    inv = lambda x: pow(x, r - 2, r)
    y, z, e = ch[0], ch[1], ch[2]
    rest = alpha_k(r, n, m, ch, blind, [0] + list(gammas[1:]))
    c0 = pow(y, n * m + 1, r) * (pow(z, 2, r) if m > 1 else 1) % r
    return ((target - blind[4] - blind[3] * e) * inv(e * e) - rest) * inv(c0) % r


# ---- the many-key form, in big integers ----------------------------------------------------------------------------------
def coeff_closed_forms(r, n, m, dprime, ch):
    """[A0, c_alpha, c_delta, c_eta, c_dL[0..k), c_dR[0..k)] with D = (y^(nm+1) [z^2])^-1 (csrc/recover_coeffs.hpp's head
    comment, written out): -D, -D e^-1, -D e^-2, -D e_t^2, -D e_t^-2 and A0 = D e^-2 delta'.  No challenge may be zero."""
    inv = lambda x: pow(x, r - 2, r)
    y, z, e, et = ch[0], ch[1], ch[2], ch[3:]
    D = inv(pow(y, n * m + 1, r) * (z * z if m > 1 else 1) % r)
    return [D * inv(e * e) * dprime % r, -D % r, -D * inv(e) % r, -D * inv(e * e) % r] + \
        [-D * x * x % r for x in et] + [-D * inv(x * x) % r for x in et]


def gamma_by_coeffs(r, coeffs, blind):
    """A0 + sum c_s slot_s over the live slots alpha, delta, eta, d_L, d_R of the blinding scalars `blind`"""
    live = [blind[0], blind[3], blind[4]] + list(blind[5:])
    assert len(live) == len(coeffs) - 1
    return (coeffs[0] + sum(c * s for c, s in zip(coeffs[1:], live))) % r


# ---- rows ----------------------------------------------------------------------------------------------------------------
class Row:
    """cname, n, m, k, name, source ("buffer" | "key"), key, index (key rows), blind [5 + 2k ints] (a key row's: the
    expansion), gammas, ch, triple [r', s', delta'] (r', s': junk, the recovery reads neither), gamma (expected), bad (the
    expected flag)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "<%s (%d,%d) %s %s>" % (self.cname, self.n, self.m, self.name, self.source)


def make_row(cname, n, m, name, source, index=0, key=OWNER):
    """the named row of a shape; a key row's blinding is blinding_from_key(key, index); deterministic in its arguments"""
    r = RC.ORDER[cname]
    k = log2(n * m)
    if name not in row_names(k, source):
        raise ValueError("no row %r at k = %d from a %s" % (name, k, source))
    rng = random.Random("%s/%d/%d/%s/%s/%d" % (cname, n, m, name, source, index))
    nz = lambda: rng.randrange(1, r)
    if source == "key":
        blind = RC.O.blinding_from_key(key, index, k, r)
    else:
        blind = [rng.randrange(r) for _ in range(5 + 2 * k)]
    ch = [nz() for _ in range(3 + k)]
    gammas = [rng.randrange(r) for _ in range(m)]
    if name == "minus_one":
        ch = [r - 1] * (3 + k)
    elif name == "one":
        ch = [1] * (3 + k)
    elif name.startswith("top("):
        i, top = int(name[4:-1]), top_values(r)
        ch = [top[(i * (3 + k) + s) % TOP_VALUES] for s in range(3 + k)]
    elif name.startswith("blind_edges("):
        i = int(name[12:-1])
        blind = [(0, 1, r - 1)[(s + i) % 3] for s in range(5 + 2 * k)]
        blind[1], blind[2] = nz(), nz()   # r and s: coefficient zero
    elif name == "gamma_zero":
        gammas = [0] * m
    elif name.startswith("delta_edges("):
        target = int(name[12:-1]) % r
        gammas[0] = solve_gamma0(r, n, m, ch, blind, gammas, target)
    dprime = delta_prime(r, n, m, ch, blind, gammas)
    if name.startswith("delta_edges("):
        assert dprime == int(name[12:-1]) % r
    gamma, bad = RC.gamma_of(r, gammas, ch[1]), False
    if is_zero_name(name):
        pos = zero_position(name, k)
        ch[pos] = 0   # after delta' was built: the row keeps the non-zero row's delta'
        if pos == 1 and m == 1:
            gamma = gammas[0]   # z is not read at m = 1
        else:
            gamma, bad = 0, True
    return Row(cname=cname, n=n, m=m, k=k, name=name, source=source, key=key if source == "key" else None,
               index=index if source == "key" else None, blind=blind, gammas=gammas, ch=ch,
               triple=[nz(), nz(), dprime], gamma=gamma, bad=bad)


def shape_rows(cname, n, m, source, index0=0, names=None):
    """every named row of one shape (or `names`), key rows at the indices index0, index0 + 1, .."""
    names = row_names(log2(n * m), source) if names is None else names
    return [make_row(cname, n, m, name, source, index0 + i) for i, name in enumerate(names)]


def corpus(cname, source):
    """every named row of every shape of shapes(k), k = 0..12"""
    out = []
    for k in KS:
        for n, m in shapes(k):
            out += shape_rows(cname, n, m, source, (1 << 32) - 7 + 100 * k)
    return out


def mixed_items(n, ms, source, per_class=None):
    """[(m, name)]: the named rows (or the first per_class of them) of the shapes (n, m), m in ms, dealt round-robin so that
    the m_of of a call cycles through ms and its packed offsets advance by a different amount per proof"""
    lists = [[(m, name) for name in row_names(log2(n * m), source)[:per_class]] for m in ms]
    out = []
    for i in range(max(len(x) for x in lists)):
        out += [x[i] for x in lists if i < len(x)]
    return out


def foreign_gamma(row, key, index):
    """what another key reads out of a non-zero row: the inverse direction on ITS expansion, through the closed forms"""
    r = RC.ORDER[row.cname]
    return gamma_by_coeffs(r, coeff_closed_forms(r, row.n, row.m, row.triple[2], row.ch),
                           RC.O.blinding_from_key(key, index, row.k, r))
