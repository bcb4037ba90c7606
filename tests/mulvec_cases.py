"""Shared case builder of the back-end tests (CPU: test_mulvec_cases_cpu.py, GPU: test_gpu_mulvec_backend.py): batches of
MulVec scalars and proof records for bpp_debug_verifier_mulvec, with the result the DEFINITION gives each record.  Nothing
here imports the product: the cases are built with oracle/ and pyref alone.

The reference is big-integer arithmetic.  The key is pyref.PublicKey's -- g, h = 2 g, G_i = 3 (i + 1) g, H_i = 5 (i + 1) g --
and every proof point is a known multiple a g, so record r's MulVec is the one group element E_r g with
    E_r = sum_t S_r[t] dlog(point_t) mod r          (infinity: dlog 0)
over the terms in MULVEC ORDER: head (3), g, h, L (k), R (k), G (mn), H (mn), V (m); the head is [A, wip.A, wip.B] of the
record for m > 1 and reversed for m = 1.  The expected wire point is one oracle scalar multiplication of g, the expected
verdict 0 iff E_r = 0.

A batch cycles through the record classes by GLOBAL record index gi = offset + i: class CLASSES[gi % len], variant
gi // len.  batch(..., classes=("one_hot",)) is the sweep of the single non-zero term: record gi has scalar 1 (gi even) or
r - 1 (gi odd) on term (gi // 2) % N.

hashed=True builds the same scalars over points whose discrete logs nobody knows: the caller supplies the pool of wire
points (pool_wire) and gets no E; the classes that solve for a scalar (cancel, near_miss) are left out.
"""

import functools
import random

import numpy as np

import glv_cases as GC
import oracle as O
import pyref as P
from verdict_corpus import CID, FastEdwards

Z2, HALF_MAX = GC.Z2, GC.HALF_MAX

CLASSES = ("random", "all_zero", "fixed_only", "proof_only", "one_hot", "all_one", "all_minus_one", "digits", "small",
           "z2_multiples", "nibbles", "cancel", "near_miss", "points")
NEEDS_DLOG = ("cancel", "near_miss")

# the pool of proof points: 24 random multiples of g, then 1 g .. 8 g, then G_0 (= 3 g)
POOL_RANDOM = 24
POOL_SMALL = POOL_RANDOM          # index of 1 g; j g sits at POOL_SMALL + j - 1
POOL_G0 = POOL_RANDOM + 8
POOL_SIZE = POOL_G0 + 1
INF = -1                          # token index of the point at infinity (wire flag)
POINT_VARIANTS = 12


def classes_of(cname, hashed=False):
    cl = [c for c in CLASSES if c != "z2_multiples" or cname == "bls12_381"]
    return tuple(c for c in cl if not (hashed and c in NEEDS_DLOG))


# ---- the window layouts, restated ----------------------------------------------------------------------------------
def glv_layout(c, fr_bits=255, hmax=HALF_MAX):
    """csrc/fixed_glv.hpp glv_layout: (widths of the W - 1 signed windows, offsets of all W windows, top, bias)"""
    W = ((fr_bits - 1) // c + 1) // 2
    ns = W - 1
    assert 2 <= W <= 64
    best = None
    for S in range(ns, 128):
        q, rem = divmod(S, ns)
        if q + (1 if rem else 0) > 24:
            break
        widths = [q + (1 if j >= ns - rem else 0) for j in range(ns)]   # the wider windows on top
        offs = [sum(widths[:j]) for j in range(W)]
        bias = sum(1 << (o + w - 1) for o, w in zip(offs, widths))
        top = (hmax + bias) >> S
        entries = sum(1 << (w - 1) for w in widths) + top
        if top == 0 or top >> 31 or entries >> 32:
            continue
        if best is None or entries < best[0]:
            best = (entries, widths, offs, top, bias)
    return best[1:]


def balanced_split(k):
    """csrc/ec.hpp glv_split_balanced on BLS12-381: k = s1 k1 + s2 k2 z^2 (mod r) as the signed pair (s1 k1, s2 k2)"""
    R = GC.R
    above = k > (R - 1) // 2
    kk = R - k if above else k
    k1, k2 = kk % Z2, kk // Z2
    big = 2 * k1 > Z2
    if big:
        k1, k2 = Z2 - k1, k2 + 1
    return (-k1 if above != big else k1), (-k2 if above else k2)


def recode_mixed(h, widths, offs, bias):
    """the digits of a half h >= 0 under a GLV layout: the bias trick of fixed_glv.hpp"""
    v = h + bias
    d = [((v >> o) & ((1 << w) - 1)) - (1 << (w - 1)) for o, w in zip(offs, widths)]
    return d + [v >> offs[-1]]


def recode_uniform(k, c, W):
    """the digits of a scalar under the unsplit layout (csrc/fixed_glv.hpp win_layout_uniform, k_fixed_msm): W - 1 signed windows
    of c bits, then what is left"""
    half = 1 << (c - 1)
    v = k + sum(half << (c * j) for j in range(W - 1))
    return [((v >> (c * j)) & ((1 << c) - 1)) - half for j in range(W - 1)] + [v >> (c * (W - 1))]


def recode_nibbles(k, windows):
    """k_var_digits: digit j = nibble j of (k + 0x88..8) - 8"""
    v = k + sum(8 << (4 * j) for j in range(windows))
    return [((v >> (4 * j)) & 15) - 8 for j in range(windows)]


class Shape:
    """one pass shape: (n, m) is the shape of the PASS -- a prefix view's m', not the m of the verifier that owns the tables"""

    def __init__(self, cname, n, m, c):
        self.cname, self.cid, self.n, self.m, self.c = cname, CID[cname], n, m, c
        self.curve = P.CURVES[cname]
        self.r = self.curve["r"]
        self.mn = n * m
        self.k = self.mn.bit_length() - 1
        assert 1 << self.k == self.mn
        self.N, self.NF, self.NV = 2 * self.mn + 2 * self.k + m + 5, 2 * self.mn + 2, 3 + 2 * self.k + m
        self.L = O.fp_limbs(self.cid)
        self.PW = 2 * self.L + 1
        self.glv = cname == "bls12_381"          # kernels.hpp fixed_glv<C>()
        self.var_glv = cname != "ed25519"         # the proof points' scalars are split too (2 x 33 nibbles)
        if self.glv:
            self.widths, self.offs, self.top, self.bias = glv_layout(c)
            self.W = len(self.offs)
        else:
            self.W = (self.r.bit_length() - 1) // c + 1
            self.half = 1 << (c - 1)
            self.top = recode_uniform(self.r - 1, c, self.W)[-1]
        self.mu = Z2 if self.glv else (GC.SECP_LAMBDA if self.var_glv else None)

    def fixed_term_index(self, f):
        return 3 + f if f < 2 else 5 + 2 * self.k + (f - 2)

    def var_term_index(self, v):
        if v < 3:
            return 2 - v if self.m == 1 else v
        if v < 3 + 2 * self.k:
            return 5 + (v - 3)
        return 5 + 2 * self.k + 2 * self.mn + (v - 3 - 2 * self.k)

    @property
    def fixed_terms(self):
        return [self.fixed_term_index(f) for f in range(self.NF)]

    @property
    def proof_terms(self):
        return [self.var_term_index(v) for v in range(self.NV)]

    def fixed_dlogs(self):
        """dlog of fixed generator f: g, h, G_0.., H_0.. (pyref.PublicKey).

        These dlogs collide: G_4 = 15 g = H_2, G_9 = H_5, .., and the pool's 1 g, 2 g, 3 g are g, h and G_0.  Two generators of
        equal dlog are the same point, so no record over this key -- the one_hot sweep included -- can tell a map that
        swapped exactly such a pair from the right one.  Only the hashed-key cases, whose points are all distinct, can,
        and they run at NF = 10.  A swap of any other pair changes E."""
        return [1, 2] + [3 * (i + 1) for i in range(self.mn)] + [5 * (i + 1) for i in range(self.mn)]


# ---- the chosen scalars -----------------------------------------------------------------------------------------------
def _from_digits(d, offs):
    return sum(x << o for x, o in zip(d, offs))


@functools.lru_cache(maxsize=None)
def digit_scalars(cname, c):
    """the `digits` class: [(scalar, claim)]; claim None, or the digits the scalar must recode to -- a list of W digits
    (unsplit layout), or ((signed k1, its digits), (signed k2, its digits)) under the GLV layout"""
    sh = Shape(cname, 2, 2, c)
    r, W = sh.r, sh.W
    out = []
    if not sh.glv:
        half, offs = sh.half, [c * j for j in range(W)]
        lo, hi = [-half] * (W - 1), [half - 1] * (W - 1)
        alt = [(-half if j % 2 == 0 else half - 1) for j in range(W - 1)]
        alt2 = [(half - 1 if j % 2 == 0 else -half) for j in range(W - 1)]
        hi_top = min(sh.top, (r - 1 - _from_digits(hi, offs)) >> offs[-1])   # the largest top digit that stays below r
        fit = lambda d: d + [0 if _from_digits(d, offs[:-1]) >= 0 else 1]   # the smallest top digit that makes it a scalar
        for d in (fit(lo), fit(hi), hi + [hi_top], fit(alt), fit(alt2), lo + [sh.top]):
            k = _from_digits(d, offs)
            assert 0 <= k < r and recode_uniform(k, c, W) == d, (cname, c, d)
            out.append((k, list(d)))
        out.append((r - 1, recode_uniform(r - 1, c, W)))     # the largest top digit there is
        out += [(k, None) for k in (0, 1, 2, r - 2)]
        if cname == "secp256k1":
            ks = GC.secp_split_scalars()
            out += [(k, None) for k in ks[:15] + ks[-16:]]   # its edges (the 4000 random scalars sit between them)
        return out
    widths, offs, bias = sh.widths, sh.offs, sh.bias
    lo = [-(1 << (w - 1)) for w in widths]
    hi = [(1 << (w - 1)) - 1 for w in widths]
    alt = [(lo[j] if j % 2 == 0 else hi[j]) for j in range(W - 1)]
    alt2 = [(hi[j] if j % 2 == 0 else lo[j]) for j in range(W - 1)]

    def half_of(d):
        t = 0 if _from_digits(d, offs) >= 0 else 1
        h = _from_digits(d + [t], offs)
        # both halves within what the balanced split returns unchanged: k1 <= z^2 / 2, k2 <= z^2 / 2 - 1
        assert 0 <= h <= Z2 // 2 - 1, (c, d)
        assert recode_mixed(h, widths, offs, bias) == d + [t]
        return h, d + [t]

    pats = [half_of(d) for d in (lo, hi, alt, alt2)]
    pairs = [(p, p) for p in pats] + [(pats[0], pats[1]), (pats[1], pats[0])]
    for (h1, d1), (h2, d2) in pairs:
        for s1 in (1, -1):
            for s2 in (1, -1):
                out.append(((s1 * h1 + s2 * h2 * Z2) % r, ((s1 * h1, d1), (s2 * h2, d2))))
    out += [(k, None) for k in GC.edges()]
    grid = (0, 1, -1, HALF_MAX - 1, -(HALF_MAX - 1), HALF_MAX, -HALF_MAX)
    out += [((k1 + k2 * Z2) % r, None) for k1 in grid for k2 in grid]
    return out


@functools.lru_cache(maxsize=None)
def nibble_scalars(cname):
    """the `nibbles` class (proof terms): [(scalar, claim)]; claim None or the 65 digits of the unsplit recoding"""
    sh = Shape(cname, 2, 2, 4)
    r = sh.r
    out = []
    if not sh.var_glv:
        offs = [4 * j for j in range(65)]
        for d in ([-8] * 63 + [1, 0], [7] * 63 + [0, 0], [-8, 7] * 31 + [-8, 1, 0], [7, -8] * 31 + [7, 0, 0]):
            k = _from_digits(d, offs)
            assert 0 <= k < r
            out.append((k, d))
        for k in (1 << 252, (1 << 252) + 1, (1 << 252) - 1, r - 1, r - 2):   # window 63 (bits 252..255) non-zero
            out.append((k, recode_nibbles(k, 65)))
        assert out[-2][1][63] == 1
    else:
        nib7 = int("7" * 32, 16)
        nib8 = (1 << 128) - int("8" * 32, 16)            # 32 digits -8, then 1
        assert recode_nibbles(nib8, 33) == [-8] * 32 + [1] and recode_nibbles(nib7, 33) == [7] * 32 + [0]
        halves = [nib7, nib8, (1 << 128) - 1, 1] + [8 << (4 * j) for j in range(32)] + [(1 << (4 * j)) - 1 for j in (1, 16, 31, 32)]
        # the pattern runs fastest: a batch reads this list cyclically from its start, and the first len(halves) entries
        # already put every pattern -- 8 * 16^j of every window j among them -- on both halves at once
        for pick in (lambda h: (h, h), lambda h: (h, 0), lambda h: (0, h), lambda h: (h, 1), lambda h: (1, h)):
            for s1, s2 in ((1, 1),) if cname == "bls12_381" else ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                for h in halves:
                    h1, h2 = pick(h)
                    k = s1 * h1 + s2 * h2 * sh.mu
                    if cname == "bls12_381" and not (h1 < Z2 and k < r):
                        continue                      # not the split's own (remainder, quotient)
                    out.append((k % r, None))
        out.append((r - 1, None))
    full = [int("7" * 64, 16), int("8" * 64, 16), int("87" * 32, 16), int("78" * 32, 16)]
    full += [8 << (4 * j) for j in range(64)] + [(1 << (4 * j)) - 1 for j in range(1, 65)]
    out += [(k % r, None) for k in full]
    return out


# ---- the points -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _group(cname):
    return FastEdwards(P.CURVES[cname]) if cname == "ed25519" else P.WeierstrassGroup(P.CURVES[cname])


_WIRE = {}


def wire_of_dlog(cname, a):
    """the wire point a g (one oracle scalar multiplication, remembered); a = 0: infinity"""
    cid, r = CID[cname], P.CURVES[cname]["r"]
    a %= r
    key = (cname, a)
    if key not in _WIRE:
        if a == 0:
            w = O.point_to_wire(cid, None)
        elif (cname, r - a) in _WIRE:
            w = O.point_to_wire(cid, _group(cname).neg(O.wire_to_point(cid, _WIRE[(cname, r - a)])))
        elif cname == "ed25519":
            G = _group(cname)
            w = O.point_to_wire(cid, G.mul(G.base(), a))
        else:
            w = O.point_mul(cid, O.generator(cid), a)
        _WIRE[key] = w
    return _WIRE[key]


@functools.lru_cache(maxsize=None)
def pool_dlogs(cname):
    rng = random.Random("mulvec pool " + cname)
    r = P.CURVES[cname]["r"]
    return [rng.randrange(1, r) for _ in range(POOL_RANDOM)] + list(range(1, 9)) + [3]


@functools.lru_cache(maxsize=None)
def _pool_wire(cname):
    return np.stack([wire_of_dlog(cname, a) for a in pool_dlogs(cname)])


@functools.lru_cache(maxsize=None)
def _negated(cname, pool_bytes):
    cid = CID[cname]
    pool = np.frombuffer(pool_bytes, dtype=np.uint64).reshape(POOL_SIZE, -1)
    return np.stack([O.point_to_wire(cid, _group(cname).neg(O.wire_to_point(cid, w))) for w in pool])


def key_wire(cname, mn):
    """(gh, G, H) of pyref.PublicKey(mn) in wire form"""
    sh = Shape(cname, mn, 1, 4)
    w = np.stack([wire_of_dlog(cname, a) for a in sh.fixed_dlogs()])
    return w[:2], w[2:2 + mn], w[2 + mn:]


def mulvec_points(sh, gh, G, H, rec):
    """the points of one record's MulVec in the order of its scalars"""
    head = rec[:3][::-1] if sh.m == 1 else rec[:3]
    k = sh.k
    return np.concatenate([head, gh, rec[3:3 + 2 * k], G[:sh.mn], H[:sh.mn], rec[3 + 2 * k:]])


# ---- one record -------------------------------------------------------------------------------------------------------
def _record(sh, cls, j, rng, hashed):
    """(scalars in MulVec order, tokens (pool index or INF, negated) in RECORD order, note)"""
    r, N, NV = sh.r, sh.N, sh.NV
    fixed, proof = sh.fixed_terms, sh.proof_terms
    toks = [(i, False) for i in rng.sample(range(POOL_RANDOM), min(NV, POOL_RANDOM))]
    toks += [(rng.randrange(POOL_RANDOM), False) for _ in range(NV - len(toks))]
    S = [rng.randrange(r) for _ in range(N)]
    note = None
    if cls == "random":
        pass
    elif cls == "all_zero":
        S = [0] * N
    elif cls == "fixed_only":
        for t in proof:
            S[t] = 0
    elif cls == "proof_only":
        for t in fixed:
            S[t] = 0
    elif cls == "one_hot":
        t = (j // 2) % N
        S = [0] * N
        S[t] = 1 if j % 2 == 0 else r - 1
        note = t
    elif cls == "all_one":
        S = [1] * N
    elif cls == "all_minus_one":
        S = [r - 1] * N
    elif cls == "digits":
        ds = digit_scalars(sh.cname, sh.c)
        S = [ds[(j * N + t) % len(ds)][0] for t in range(N)]
    elif cls == "small":
        S = [rng.randrange(1 << 64) for _ in range(N)]
    elif cls == "z2_multiples":
        S = [(rng.randrange(1 << 126) if t % 3 else t) * Z2 for t in range(N)]
        assert max(S) < r
    elif cls == "nibbles":
        ns = nibble_scalars(sh.cname)
        for v, t in enumerate(proof):
            S[t] = ns[(j * NV + v) % len(ns)][0]
    elif cls in ("cancel", "near_miss"):
        pass                                          # the scalar on g is solved by the caller, who knows the dlogs
    elif cls == "points":
        var = j % POINT_VARIANTS
        note = var
        k = sh.k
        L0, R0 = 3, 3 + k
        equal = var % 2 == 1
        if var in (0, 1):                             # L_0 == R_0
            toks[R0] = toks[L0]
            pair = (L0, R0)
        elif var in (2, 3):                           # L_0 == -R_0: with equal scalars every window sum cancels
            toks[R0] = (toks[L0][0], True)
            pair = (L0, R0)
        elif var in (4, 5):                           # a proof point equal to G_0
            toks[0] = (POOL_G0, False)
            pair = (0, None)
            if equal:
                S[sh.var_term_index(0)] = S[sh.fixed_term_index(2)]
        elif var in (6, 7):                           # 1 g .. 8 g together: their tables of 1 P .. 8 P coincide
            cnt = min(8, NV - 3)
            for i in range(cnt):
                toks[3 + i] = (POOL_SMALL + i, False)
            pair = None
            if equal:
                for i in range(cnt):
                    S[sh.var_term_index(3 + i)] = S[sh.var_term_index(3)]
        elif var in (8, 9):                           # infinity (wire flag) carrying a non-zero scalar
            toks[L0 if var == 8 else NV - 1] = (INF, False)
            pair = None
        else:                                         # every proof point the same P (10), or P, -P, P, .. (11): equal scalars
            toks = [(toks[0][0], var == 11 and v % 2 == 1) for v in range(NV)]
            for v in range(NV):
                S[sh.var_term_index(v)] = S[sh.var_term_index(0)]
            pair = None
        if pair and pair[1] is not None and equal:
            S[sh.var_term_index(pair[1])] = S[sh.var_term_index(pair[0])]
        if var in (8, 9):
            assert S[sh.var_term_index(L0 if var == 8 else NV - 1)] != 0
    else:
        raise KeyError(cls)
    return S, toks, note


class Batch:
    """scalars_int [count][N], tokens [count][NV], cls / note per record; scalars (count, N, 4) and records (count, NV, PW)
    u64; known dlogs: dlogs [count][N] and E [count], expect_ok (count,) u32, expect_result (count, PW) u64"""


def _scalars_wire(rows):
    buf = b"".join(x.to_bytes(32, "little") for row in rows for x in row)
    return np.frombuffer(buf, dtype=np.uint64).reshape(len(rows), -1, 4).copy()


def batch(cname, n, m, c, count, offset=0, classes=None, hashed=False, pool_wire=None, seed=0):
    """`count` records of pass shape (n, m) at window_bits c, global record indices offset .. offset + count - 1"""
    sh = Shape(cname, n, m, c)
    cl = classes_of(cname, hashed) if classes is None else tuple(classes)
    r = sh.r
    b = Batch()
    b.shape, b.classes = sh, cl
    b.cls, b.note, b.scalars_int, b.tokens = [], [], [], []
    if hashed:
        pool = np.ascontiguousarray(pool_wire, dtype=np.uint64)
        assert pool.shape == (POOL_SIZE, sh.PW)
        dl = None
    else:
        dl = pool_dlogs(cname)
        pool = _pool_wire(cname)
    neg_pool = _negated(cname, pool.tobytes())
    inf = O.point_to_wire(sh.cid, None)
    fd = sh.fixed_dlogs()
    b.E, b.dlogs = (None, None) if hashed else ([], [])
    recs = np.zeros((count, sh.NV, sh.PW), dtype=np.uint64)
    for i in range(count):
        gi = offset + i
        cls, j = cl[gi % len(cl)], gi // len(cl)
        rng = random.Random("%s %d %d %d %d %d" % (cname, n, m, c, seed, gi) + cls)
        S, toks, note = _record(sh, cls, j, rng, hashed)
        if not hashed:
            D = [0] * sh.N
            for f in range(sh.NF):
                D[sh.fixed_term_index(f)] = fd[f]
            for v, (pi, ng) in enumerate(toks):
                a = 0 if pi == INF else dl[pi]
                D[sh.var_term_index(v)] = (r - a) % r if ng else a
            if cls in ("cancel", "near_miss"):
                gt = sh.fixed_term_index(0)
                S[gt] = 0
                S[gt] = (-sum(s * d for s, d in zip(S, D)) + (1 if cls == "near_miss" else 0)) % r
            b.E.append(sum(s * d for s, d in zip(S, D)) % r)
            b.dlogs.append(D)
        for v, (pi, ng) in enumerate(toks):
            recs[i, v] = inf if pi == INF else (neg_pool[pi] if ng else pool[pi])
        assert all(0 <= s < r for s in S)
        b.cls.append(cls)
        b.note.append(note)
        b.scalars_int.append(S)
        b.tokens.append(toks)
    b.records = recs
    b.scalars = _scalars_wire(b.scalars_int)
    if not hashed:
        b.expect_ok = np.array([1 if e else 0 for e in b.E], dtype=np.uint32)
        b.expect_result = np.stack([wire_of_dlog(cname, e) for e in b.E])
    return b


# ---- the shapes of the GPU test: (curve, n, m of the verifier, window_bits, count, m_view, Horner form, blocks per proof) ----
# Form and blocks are what impl_verify.hpp's horner_form and blocks_per_proof give (3 = the lone form of the tree); the GPU
# test holds the hook's out_geometry to them.  With FIXED_BLOCK = 128: blocks = ceil(min(2^18 / count, NF) / 128), the tree
# up to 256 proofs, lone while count * blocks <= 1024, and above 256 proofs eight lanes per proof while
# count (NF adds / 7e9 + 9.2e-8) < 2e-3 (adds = W, or 2 W under the GLV layout).
# NF = 258 has at most 3 blocks, so 256 proofs never leave the lone form: the tree that is not lone needs NF = 514 (n m = 256),
# whose 5 blocks pass 1024 at 205 proofs.
GPU_CASES = [
    # lone tree, NF = 10: lanes without a generator
    ("bls12_381", 2, 2, 3, 1, 0, 3, 1), ("bls12_381", 2, 2, 3, 3, 0, 3, 1), ("bls12_381", 2, 2, 3, 64, 0, 3, 1),
    ("secp256k1", 2, 2, 3, 1, 0, 3, 1), ("secp256k1", 2, 2, 3, 3, 0, 3, 1), ("secp256k1", 2, 2, 3, 64, 0, 3, 1),
    ("ed25519", 2, 2, 3, 1, 0, 3, 1), ("ed25519", 2, 2, 3, 3, 0, 3, 1), ("ed25519", 2, 2, 3, 64, 0, 3, 1),
    # NF = 66; window counts of both parities per half (W = 18, 13, 12 on BLS12-381)
    ("bls12_381", 4, 8, 7, 64, 0, 3, 1), ("secp256k1", 16, 2, 9, 64, 0, 3, 1), ("ed25519", 4, 8, 7, 64, 0, 3, 1),
    ("bls12_381", 4, 8, 10, 64, 0, 3, 1), ("bls12_381", 4, 8, 11, 64, 0, 3, 1),
    # NF = 258: three blocks per proof and no spreading; two blocks (G = 1 and 2 left-over generators); one block (G = 2 and
    # 2 left-over) -- the last two in the one-lane-per-proof form
    ("bls12_381", 16, 8, 4, 3, 0, 3, 3), ("secp256k1", 16, 8, 4, 3, 0, 3, 3),
    ("bls12_381", 16, 8, 4, 1100, 0, 0, 2), ("secp256k1", 16, 8, 4, 1100, 0, 0, 2), ("ed25519", 16, 8, 4, 1100, 0, 0, 2),
    ("bls12_381", 16, 8, 4, 2100, 0, 0, 1), ("secp256k1", 16, 8, 4, 2100, 0, 0, 1), ("ed25519", 16, 8, 4, 2100, 0, 0, 1),
    # eight lanes per proof; 257 and 300 leave a last block with one and with twelve proofs
    ("bls12_381", 8, 2, 5, 257, 0, 2, 1), ("bls12_381", 8, 2, 5, 300, 0, 2, 1),
    ("ed25519", 8, 2, 5, 257, 0, 2, 1), ("ed25519", 8, 2, 5, 300, 0, 2, 1),
    # the tree that is not lone: 205 x 5 = 1025 blocks
    ("bls12_381", 32, 8, 4, 205, 0, 1, 5), ("ed25519", 32, 8, 4, 205, 0, 1, 5),
    # prefix views of an m = 8 table
    ("bls12_381", 4, 8, 7, 64, 1, 3, 1), ("bls12_381", 4, 8, 7, 64, 4, 3, 1),
    ("secp256k1", 4, 8, 7, 64, 1, 3, 1), ("secp256k1", 4, 8, 7, 64, 4, 3, 1),
]
HASHED_CASES = [("bls12_381", 2, 2, 3, 16), ("secp256k1", 2, 2, 3, 16), ("ed25519", 2, 2, 3, 16)]


def pass_shapes():
    """the distinct pass shapes (curve, n, m of the pass, window_bits) of GPU_CASES"""
    out = []
    for cname, n, m, c, _, mv, _, _ in GPU_CASES:
        t = (cname, n, mv or m, c)
        if t not in out:
            out.append(t)
    return out
