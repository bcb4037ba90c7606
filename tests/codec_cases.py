"""Shared case builder of the codec tests (CPU: test_codec_cases_cpu.py, GPU: test_gpu_codec_cases.py): the inputs at
which the point codecs (csrc/codec.hpp, csrc/ristretto.hpp) and the generator hashing (csrc/hash_to_group.hpp) take each
of their branches, with the answer of the restatement (oracle/pyref.py) and, where the code branches on values, the
TRACE: the tuple of branches the restatement took.  Nothing here imports the product; everything is deterministic.

The traces come from tracing twins of pyref's functions written here (sqrt_ratio_m1, decode, encode, MAP, the element
derivation, hash_to_group).  A twin restates its function with the branch outcomes recorded; test_codec_cases_cpu.py
holds every twin to the function it shadows on the whole corpus, and counts the traces (the census), so that "the device
equals the restatement on this corpus" is a statement about every branch and not about whichever the corpus happened to
reach.

  ristretto255 decode trace : (outcome of SQRT_RATIO_M1, root negated by its abs, x negated by its abs, t negative)
  ristretto255 encode trace : (outcome, root negated, rotate, x z_inv negative, s negated by the final abs)
  MAP trace                 : (outcome, root negated)
outcome: "correct" (v r^2 = u), "flipped" (= -u), "flipped_i" (= -u i), "none" (= u i, or u v = 0).
"""

import collections
import functools
import hashlib
import random

import pyref as P
from verdict_corpus import FastEdwards

R = P.Ristretto255
ED_P = R.P
ED_R = P.ED25519["r"]
FB = {"bls12_381": 48, "secp256k1": 32}

DecodeCase = collections.namedtuple("DecodeCase", "data point trace reason note")
EncodeCase = collections.namedtuple("EncodeCase", "point data trace coset note")
PointCase = collections.namedtuple("PointCase", "data ok point note")
HalfCase = collections.namedtuple("HalfCase", "point data above note")
HashedPoint = collections.namedtuple("HashedPoint", "point ctr flipped maps")

# why rist_decode turns a string down, in the order the checks are made
REASONS = ("bit 255 set", "non-canonical", "negative s", "not a square", "negative t", "y = 0")


# ---- tracing twins of pyref.Ristretto255 ---------------------------------------------------------------------------
def sqrt_ratio_m1_traced(u, v):
    """pyref.Ristretto255.sqrt_ratio_m1 -> (was_square, r, outcome, root negated)"""
    p = ED_P
    v3 = v * v * v % p
    v7 = v3 * v3 * v % p
    r = u * v3 * pow(u * v7, (p - 5) // 8, p) % p
    check = v * r * r % p
    if check == u % p:
        outcome = "correct"
    elif check == (-u) % p:
        outcome = "flipped"
    elif check == (-u) * R.SQRT_M1 % p:
        outcome = "flipped_i"
    else:
        outcome = "none"
    if outcome in ("flipped", "flipped_i"):
        r = R.SQRT_M1 * r % p
    negated = bool(r & 1)
    if negated:
        r = p - r
    return outcome in ("correct", "flipped"), r, outcome, negated


def decode_traced(b):
    """pyref.Ristretto255.decode -> (point or None, trace or None, reason or None); the trace exists once the string is
    a canonical non-negative s, whatever the verdict"""
    p = ED_P
    s = int.from_bytes(b, "little")
    if s >> 255:
        return None, None, "bit 255 set"
    if s >= p:
        return None, None, "non-canonical"
    if s & 1:
        return None, None, "negative s"
    ss = s * s % p
    u1, u2 = (1 - ss) % p, (1 + ss) % p
    u2s = u2 * u2 % p
    v = (-(R.D * u1 * u1) - u2s) % p
    ok, inv, outcome, root_neg = sqrt_ratio_m1_traced(1, v * u2s % p)
    den_x = inv * u2 % p
    den_y = inv * den_x * v % p
    x = 2 * s * den_x % p
    x_neg = bool(x & 1)
    if x_neg:
        x = p - x
    y = u1 * den_y % p
    t = x * y % p
    trace = (outcome, root_neg, x_neg, bool(t & 1))
    if not ok:
        return None, trace, "not a square"
    if t & 1:
        return None, trace, "negative t"
    if y == 0:
        return None, trace, "y = 0"
    return (x, y), trace, None


def encode_traced(pt):
    """pyref.Ristretto255.encode -> (32 bytes, trace)"""
    p = ED_P
    x0, y0 = (0, 1) if pt is None else pt
    t0 = x0 * y0 % p
    u1 = (1 + y0) * (1 - y0) % p
    u2 = x0 * y0 % p
    _, inv, outcome, root_neg = sqrt_ratio_m1_traced(1, u1 * u2 * u2 % p)
    den1, den2 = inv * u1 % p, inv * u2 % p
    z_inv = den1 * den2 * t0 % p
    rotate = bool(t0 * z_inv % p & 1)
    if rotate:
        x, y, den_inv = y0 * R.SQRT_M1 % p, x0 * R.SQRT_M1 % p, den1 * R.INVSQRT_A_MINUS_D % p
    else:
        x, y, den_inv = x0, y0, den2
    x_neg = bool(x * z_inv % p & 1)
    if x_neg:
        y = (-y) % p
    s = den_inv * (1 - y) % p
    s_neg = bool(s & 1)
    if s_neg:
        s = p - s
    return s.to_bytes(32, "little"), (outcome, root_neg, rotate, x_neg, s_neg)


def map_traced(t):
    """pyref.Ristretto255.map -> ((X, Y, Z, T), (outcome, root negated))"""
    p = ED_P
    r = R.SQRT_M1 * t * t % p
    u = (r + 1) * R.ONE_MINUS_D_SQ % p
    v = (-1 - r * R.D) * (r + R.D) % p
    ok, s, outcome, root_neg = sqrt_ratio_m1_traced(u, v)
    if not ok:
        s = (-R.ct_abs(s * t)) % p
    c = (p - 1) if ok else r
    N = (c * (r - 1) * R.D_MINUS_ONE_SQ - v) % p
    w0 = 2 * s * v % p
    w1 = N * R.SQRT_AD_MINUS_ONE % p
    w2, w3 = (1 - s * s) % p, (1 + s * s) % p
    return (w0 * w3 % p, w2 * w1 % p, w1 * w3 % p, w0 * w2 % p), (outcome, root_neg)


def from_uniform_bytes_traced(b, G):
    """pyref.Ristretto255.from_uniform_bytes -> (affine point, the two MAP traces)"""
    p = ED_P
    out, traces = [], []
    for h in range(2):
        t = int.from_bytes(b[32 * h:32 * h + 32], "little") & ((1 << 255) - 1)
        (X, Y, Z, _), tr = map_traced(t % p)
        zi = pow(Z, -1, p)
        out.append((X * zi % p, Y * zi % p))
        traces.append(tr)
    return G.add(out[0], out[1]), tuple(traces)


def h2g_digest(curve, label, kind, idx, ctr, half):
    """H(kind, idx, ctr, half) of csrc/hash_to_group.hpp, through hashlib"""
    cid = P.CURVE_IDS[curve["name"]]
    seed = hashlib.sha256(b"BulletproofsPlus-AMD generators v1\0\0" + cid.to_bytes(4, "little") + label).digest()
    return hashlib.sha256(seed + b"bppg" + b"".join(v.to_bytes(4, "little") for v in (ord(kind), idx, ctr, half))).digest()


def hash_to_group_traced(curve, G, label, kind, idx):
    """pyref.hash_to_group -> HashedPoint(point, final ctr, parity flip taken, MAP traces (ed25519) or None)"""
    if curve["name"] == "ed25519":
        pt, maps = from_uniform_bytes_traced(h2g_digest(curve, label, kind, idx, 0, 0) +
                                             h2g_digest(curve, label, kind, idx, 0, 1), G)
        return HashedPoint(pt, 0, None, maps)
    p, b = curve["p"], curve["b"]
    ctr = 0
    while True:
        x = (int.from_bytes(h2g_digest(curve, label, kind, idx, ctr, 0), "little") +
             (int.from_bytes(h2g_digest(curve, label, kind, idx, ctr, 1), "little") << 256)) % p
        rhs = (x * x * x + b) % p
        y = pow(rhs, (p + 1) // 4, p)
        if y * y % p == rhs:
            flipped = (y & 1) != (h2g_digest(curve, label, kind, idx, ctr, 2)[0] & 1)
            if flipped:
                y = p - y
            pt = (x, y)
            if curve["name"] == "bls12_381":
                pt = G.mul(pt, 0xd201000000010001)
            if pt is not None:
                return HashedPoint(pt, ctr, flipped, None)
        ctr += 1


# ---- ristretto255 corpora ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edwards():
    return FastEdwards(P.ED25519)


def _le32(v):
    return v.to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def rist_decode_cases():
    """-> tuple of DecodeCase(data, point or None, trace or None, reason or None, note)"""
    p = ED_P
    rnd = random.Random(0xC0DEC)
    vals = [(rnd.randrange(0, p, 2), "random") for _ in range(400)]
    vals += [(s, "edge") for s in (0, 2, p - 1, p - 3)]
    vals += [(s, "odd") for s in (1, 3, p - 2)]
    vals += [(s, "at or above p") for s in (p, p + 1, p + 18, (1 << 255) - 1)]
    vals += [(s, "bit 255") for s in (1 << 255, (1 << 255) + 2, (1 << 256) - 2)]
    # the three above sit over s = 0 (accepted), s = 2 (negative t) and s = 2^255 - 2 (not canonical); one more over a
    # random accepted s
    vals.append(((1 << 255) + next(s for s, _ in vals if decode_traced(_le32(s))[0] is not None and s > 2), "bit 255"))
    out = []
    for s, note in vals:
        data = _le32(s)
        _, trace, reason = decode_traced(data)
        out.append(DecodeCase(data, R.decode(data), trace, reason, note))
    return tuple(out)


TORSION = ((0, ED_P - 1), (R.SQRT_M1, 0), (ED_P - R.SQRT_M1, 0))   # E[4] without the identity


@functools.lru_cache(maxsize=None)
def rist_encode_cases():
    """-> tuple of EncodeCase(point, data, trace, coset, note): point is affine (x, y), the identity as (0, 1); the four
    cases of one coset number are the representatives P, P + (0, -1), P + (i, 0), P + (-i, 0)"""
    G = _edwards()
    rnd = random.Random(0xE2C0DE)
    ks = [0] + list(range(1, 65)) + [ED_R - 1] + [rnd.randrange(1, ED_R) for _ in range(16)]
    B = G.base()
    out = []
    for coset, k in enumerate(ks):
        Q = G.mul(B, k) if k else None
        for j, T in enumerate((None,) + TORSION):
            rep = G.add(Q, T) or (0, 1)
            _, trace = encode_traced(rep)
            out.append(EncodeCase(rep, R.encode(rep), trace, coset, "%d B + T%d" % (k, j) if k < 65 else "k B + T%d" % j))
    return tuple(out)


def uniform_cases():
    """64-byte inputs of the element derivation that only a host build reaches: hash outputs, and halves whose value t is
    in [p, 2^255) (reduced, not rejected), 0, 1, p - 1, or has bit 255 set (masked)"""
    p = ED_P
    fixed = hashlib.sha256(b"codec cases: the other half").digest()
    out = [hashlib.sha256(b"codec cases uni %d a" % i).digest() + hashlib.sha256(b"codec cases uni %d b" % i).digest()
           for i in range(64)]
    for t in list(range(p, 1 << 255)) + [0, 1, p - 1]:
        out += [_le32(t) + fixed, fixed + _le32(t)]
    top = _le32((1 << 255) | int.from_bytes(fixed, "little"))
    out += [top + fixed, fixed + top, top + top, _le32((1 << 256) - 1) + _le32(1 << 255)]
    return out


# ---- short Weierstrass corpora -------------------------------------------------------------------------------------------
def _wenc(cname, x, flag):
    """the bytes that carry x and the sign flag: BLS12-381 0x80 | flag << 5 over 48 bytes, secp256k1 02 / 03 || x"""
    if cname == "bls12_381":
        b = bytearray(x.to_bytes(48, "big"))
        assert b[0] < 0x20
        b[0] |= 0x80 | (0x20 if flag else 0)
        return bytes(b)
    return bytes([3 if flag else 2]) + x.to_bytes(32, "big")


def sweep_xs(cname):
    """the x values of the sweep: around 0, around p, around every limb (2^30j) and word (2^32j) boundary, the top"""
    p = P.CURVES[cname]["p"]
    top = 1 << (8 * FB[cname])
    fits = (1 << 381) if cname == "bls12_381" else top        # what the bytes can carry beside the flag bits
    xs = set(range(16)) | set(range(p - 16, p + 17)) | {top - 1}
    for w in (30, 32):
        j = 0
        while (1 << (w * j)) < top:
            xs |= {(1 << (w * j)) + d for d in (-1, 0, 1)}
            j += 1
    return sorted(x for x in xs if 0 <= x < fits)


@functools.lru_cache(maxsize=None)
def weierstrass_decode_cases(cname):
    """-> tuple of PointCase(data, ok, point, note): the x sweep with both flag values, then the flag cases"""
    curve = P.CURVES[cname]
    p = curve["p"]
    datas = [(_wenc(cname, x, f), "sweep") for x in sweep_xs(cname) for f in (0, 1)]
    x_off = 5
    while pow((x_off ** 3 + curve["b"]) % p, (p - 1) // 2, p) == 1:
        x_off += 1
    if cname == "bls12_381":
        for x in (0, curve["gx"], x_off):
            for top3 in range(8):
                b = bytearray(x.to_bytes(48, "big"))
                b[0] |= top3 << 5
                datas.append((bytes(b), "flags"))
    else:
        for body in (curve["gx"].to_bytes(32, "big"), bytes(32)):
            for prefix in list(range(8)) + [0xFF]:
                datas.append((bytes([prefix]) + body, "flags"))
    out = []
    for data, note in datas:
        ok, pt = P.decompress_point(curve, data)
        out.append(PointCase(data, bool(ok), pt if ok else None, note))
    return tuple(out)


def _bls_cube_root(a):
    """a cube root of a in the BLS12-381 base field, or None: p = 10 mod 27, so with t = (p - 1) / 9 and e = 1 / 3 mod t,
    (a^e)^3 = a (a^t)^k with a^t a ninth root of unity -- a^e is a cube root up to a ninth root of unity zeta^i"""
    p = P.BLS12_381["p"]
    assert p % 27 == 10
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 3, p) != 1:
        return None
    t = (p - 1) // 9
    c = pow(a, pow(3, -1, t), p)
    g = 2
    while pow(g, (p - 1) // 3, p) == 1:
        g += 1
    zeta = pow(g, t, p)
    for _ in range(9):
        if pow(c, 3, p) == a:
            return c
        c = c * zeta % p
    raise AssertionError("no cube root among the nine candidates")


@functools.lru_cache(maxsize=None)
def bls_half_cases():
    """-> tuple of HalfCase(point, data, above, note): BLS12-381 curve points (NOT in G1: for the plain codec only) whose
    y is at the boundary of words_gt_half -- (p - 1) / 2 + d, and one step of every 32-bit word away from it -- each
    followed by its negative.  note: ("bare", d) or ("word", i, sign, d)"""
    curve = P.BLS12_381
    p = curve["p"]
    half = (p - 1) // 2
    ys = [(half + d, ("bare", d)) for d in range(-8, 9)]
    for i in range(12):
        for sign in (-1, 1):
            ys += [(half + sign * (1 << (32 * i)) + d, ("word", i, sign, d)) for d in range(6)]
    out, seen = [], set()
    for y, note in ys:
        if y in seen:
            continue
        x = _bls_cube_root(y * y - 4)
        if x is None:
            continue
        seen.add(y)
        for pt, nt in (((x, y), note), ((x, p - y), ("negative",) + note)):
            out.append(HalfCase(pt, P.compress_point(curve, pt), pt[1] > half, nt))
    return tuple(out)


# ---- hashed keys -----------------------------------------------------------------------------------------------------------
LABEL = b"codec cases"
_FILL = b"SHA-256 padding boundary: 40 + len(label) bytes of seed message; 55 and 56, 63 and 64, 127 and 128 .."
assert len(_FILL) >= 88
BOUNDARY_LABELS = tuple(_FILL[:n] for n in (0, 15, 16, 23, 24, 87, 88))
KEYS = ((LABEL, 40), (LABEL, 8)) + tuple((lb, 1) for lb in BOUNDARY_LABELS)


@functools.lru_cache(maxsize=None)
def hashed_key_cases(cname):
    """-> tuple of (label, length, [h, G_0 .., H_0 ..] as HashedPoint) in the order of k_hash_to_group's lanes"""
    curve = P.CURVES[cname]
    G = _edwards() if cname == "ed25519" else P.WeierstrassGroup(curve)
    out = []
    for label, length in KEYS:
        ids = [("h", 0)] + [("G", i) for i in range(length)] + [("H", i) for i in range(length)]
        out.append((label, length, [hash_to_group_traced(curve, G, label, k, i) for k, i in ids]))
    return tuple(out)
