"""Shared case builder of the window-table tests (CPU: test_table_cases_cpu.py, GPU: test_gpu_window_tables.py): the layout of
the verifier's fixed-generator tables restated, and the entries the DEFINITION gives them,

    T[f][j][d] = [d 2^(off_j)] F_f          d = 1 .. E_j, at entry went[j] + d - 1 of generator f,

as points, as wire records and as the device's raw words.  Nothing here imports the product: the layouts are restated from
csrc/fixed_glv.hpp (GLV: mulvec_cases.glv_layout), the points come from oracle/ and pyref alone, and no discrete log is
needed, so any key will do -- hashed generators, the point at infinity, a point of small order.

Points are (x, y) tuples of integers, None the neutral element (Weierstrass infinity; the Edwards identity (0, 1), as
pyref.EdwardsGroup and the wire flag have it).

A raw coordinate is coord R mod p with R = field_cases.Field.R = 2^(30 NL), as N little-endian 32-bit words: the Montgomery
image csrc/field.hpp fe_store leaves in memory, fully reduced.  Weierstrass infinity is all zeros; the Edwards identity is the
image of x = 0, y = 1.
"""

import functools
from collections import namedtuple

import numpy as np

import field_cases as FC
import mulvec_cases as M
import oracle as O
import pyref as P
from verdict_corpus import CID, FastEdwards

TBL_RUN = 32            # csrc/kernels.hpp: entries one thread of k_tbl_fill writes
SLAB_RUNS = 1 << 21     # csrc/impl_verify.hpp create: runs one k_tbl_fill launch takes (whole generators)

Layout = namedtuple("Layout", "cname c glv W widths offs went entries top per_f runs")


# ---- the layouts, restated -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layout(cname, c):
    """widths [W] (0 for the top window), offs [W], went [W], entries [W] (the top window's is top), runs per generator"""
    r = P.CURVES[cname]["r"]
    glv = cname == "bls12_381"
    if glv:
        widths, offs, top, _ = M.glv_layout(c)
        widths, offs = list(widths), list(offs)
        W = len(offs)
    else:
        W = (r.bit_length() - 1) // c + 1
        widths, offs = [c] * (W - 1), [c * j for j in range(W)]
        bias = sum(1 << (c * j + c - 1) for j in range(W - 1))
        top = (r - 1 + bias) >> (c * (W - 1))
    entries = [1 << (w - 1) for w in widths] + [top]
    went = [sum(entries[:j]) for j in range(W)]
    if not glv:
        assert went == [j << (c - 1) for j in range(W)] and went[-1] + top == (W - 1) * (1 << (c - 1)) + top
    runs = sum(-(-e // TBL_RUN) for e in entries)
    return Layout(cname, c, glv, W, tuple(widths + [0]), tuple(offs), tuple(went), tuple(entries), top, went[-1] + top, runs)


def layout_words(L, hgap, slabs):
    """what bpp_debug_verifier_table's out_layout must hold"""
    return [L.W, L.top, L.per_f, 1 if L.glv else 0, hgap, slabs, L.runs] + list(L.widths) + list(L.went)


def slab_generators(L):
    """generators one k_tbl_fill launch takes"""
    return max(1, SLAB_RUNS // L.runs)


def max_value(cname):
    """the largest value the recoding is handed: r - 1, or the largest half of a split scalar"""
    return M.HALF_MAX if cname == "bls12_381" else P.CURVES[cname]["r"] - 1


def recode(L, v):
    if L.glv:
        _, _, _, bias = M.glv_layout(L.c)
        return M.recode_mixed(v, L.widths[:-1], L.offs, bias)
    return M.recode_uniform(v, L.c, L.W)


def sample_places(E):
    """first, second and last entries of a run, and the doubling at d = 2"""
    out = []
    for d in (1, 2, 3, 31, 32, 33, 34, 63, 64, 65, E - 1, E):
        d = min(max(d, 1), E)
        if d not in out:
            out.append(d)
    return sorted(out)


# ---- the group, through the oracle alone -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edwards():
    return FastEdwards(P.CURVES["ed25519"])


def point_mul(cname, F, k):
    """[k] F.  Weierstrass: the oracle's scalar multiplication, k reduced mod r (F of prime order); edwards25519: any F"""
    if cname == "ed25519":
        return edwards().mul(F, k)
    cid = CID[cname]
    return O.wire_to_point(cid, O.point_mul(cid, O.point_to_wire(cid, F), k % P.CURVES[cname]["r"]))


def point_add(cname, A, B):
    if cname == "ed25519":
        return P.EdwardsGroup.add(edwards(), A, B)     # pyref's affine law, not the fast one
    cid = CID[cname]
    return O.wire_to_point(cid, O.point_add(cid, O.point_to_wire(cid, A), O.point_to_wire(cid, B)))


def chain(cname, base, E):
    """base, 2 base, .. E base by repeated addition (the first step is the doubling base + base)"""
    if cname == "ed25519":
        G, out = edwards(), [base]
        for _ in range(E - 1):
            out.append(P.EdwardsGroup.add(G, out[-1], base))
        return out
    cid = CID[cname]
    bw = O.point_to_wire(cid, base)
    ws = [bw]
    for _ in range(E - 1):
        ws.append(O.point_add(cid, ws[-1], bw))
    return O.wire_to_points(cid, np.stack(ws))


def window(cname, L, F, j):
    """the E_j entries of window j of generator F: base_j = [2^off_j] F, then the chain"""
    base = point_mul(cname, F, 1 << L.offs[j]) if F is not None else None
    return chain(cname, base, L.entries[j])


def window_by_additions(cname, L, F, j):
    """the same with nothing but the addition law (a point outside the prime-order subgroup): off_j doublings, then the chain"""
    base = F
    for _ in range(L.offs[j]):
        base = point_add(cname, base, base)
    return chain(cname, base, L.entries[j])


def generator_table(cname, L, F, by_additions=False):
    """all per_f entries of one generator, in table order"""
    out = []
    for j in range(L.W):
        out += (window_by_additions if by_additions else window)(cname, L, F, j)
    assert len(out) == L.per_f
    return out


def entry(cname, L, F, j, d):
    """one entry by scalar multiplication: [d << off_j] F"""
    return None if F is None else point_mul(cname, F, d << L.offs[j])


# ---- images ----------------------------------------------------------------------------------------------------------
def base_field(cname):
    return FC.FIELDS[cname + "_fp"]


def raw_image(cname, pts):
    """(len, 2 N) uint32: the device words of the entries"""
    f = base_field(cname)
    nb = 4 * f.N
    neutral = (0, 1) if cname == "ed25519" else None
    buf = bytearray()
    for pt in pts:
        pt = neutral if pt is None else pt
        if pt is None:
            buf += bytes(2 * nb)
        else:
            buf += (pt[0] * f.R % f.p).to_bytes(nb, "little") + (pt[1] * f.R % f.p).to_bytes(nb, "little")
    return np.frombuffer(bytes(buf), dtype=np.uint32).reshape(len(pts), 2 * f.N).copy()


def raw_coordinates(cname, raw):
    """the coordinates of raw words as integers: (len, 2) objects, still in Montgomery form"""
    f = base_field(cname)
    raw = np.ascontiguousarray(raw, dtype=np.uint32).reshape(-1, 2 * f.N)
    return [(int.from_bytes(r[:f.N].tobytes(), "little"), int.from_bytes(r[f.N:].tobytes(), "little")) for r in raw]


def key_points(cname, mn):
    """the reference's key of length mn in table numbering: [g, h, G_0.., H_0..] as points"""
    gh, G, H = M.key_wire(cname, mn)
    return O.wire_to_points(CID[cname], np.concatenate([gh, G, H]))


def order8_point():
    """a point of order 8 on edwards25519, with pyref integers: the first small y that is on the curve, times l by additions
    alone, kept if four times it is not the identity"""
    c = P.CURVES["ed25519"]
    p, d, l = c["p"], c["d"], c["r"]
    G = P.EdwardsGroup(c)
    for y in range(2, 200):
        x2 = (y * y - 1) * pow(d * y * y + 1, -1, p) % p
        x = pow(x2, (p + 3) // 8, p)                       # p = 5 (mod 8)
        if (x * x - x2) % p:
            x = x * pow(2, (p - 1) // 4, p) % p
        if (x * x - x2) % p:
            continue
        T = G.mul((x, y), l)                               # LSB-first double-and-add: add alone
        if T is None:
            continue
        T2 = G.add(T, T)
        T4 = G.add(T2, T2)
        if T4 is not None:
            assert G.on_curve(T) and G.add(T4, T4) is None
            return T
    raise AssertionError("no point of order 8 found")


# ---- the cases -------------------------------------------------------------------------------------------------------
# whole tables at (n, m) = (4, 1), NF = 10: (curve, window_bits, W, entries of the signed windows, top, per_f)
WHOLE = [
    ("secp256k1", 3, 86, (4,), 2, 342),           # many short windows, runs far below 32
    ("secp256k1", 6, 43, (32,), 16, 1360),        # exactly one full run per window, half-run top
    ("secp256k1", 7, 37, (64,), 16, 2320),        # two runs per window (d0 = 33 by double-and-add)
    ("ed25519", 5, 51, (16,), 4, 804),            # Edwards chain, tiny top
    ("ed25519", 8, 32, (128,), 16, 3984),         # four runs per window, partial top run
    ("bls12_381", 4, 32, (8,), 5, 253),           # GLV table, uniform widths (all 4)
    ("bls12_381", 5, 25, (16, 32), 22, 438),      # widths 5, 6: width change, top is a partial run
    ("bls12_381", 6, 21, (32, 64), 43, 715),      # widths 6, 7: change across the run size, top = one full run + 11
]
SMALLEST = {"secp256k1": 3, "ed25519": 5, "bls12_381": 4}      # the curve's smallest row (the hashed-key cases too)
WHOLE_NM = (4, 1)
PREFIX = ("secp256k1", 4, 4, 6)                                # a verifier with prefix views: NF = 34
PREFIX_WHOLE = (0, 1, 2, 17, 18, 33)
# two slabs: (curve, n, m, window_bits, W, top, per_f, runs per generator, generators per slab, NF)
SLABS = [
    ("secp256k1", 64, 1, 16, 16, 65536, 557056, 17408, 120, 130),
    ("bls12_381", 64, 16, 13, 10, 2756, 35524, 1111, 1887, 2050),
]


def slab_samples(L, NF):
    """(generators, windows) the several-slab cases look at"""
    s = slab_generators(L)
    gens = sorted({0, 1, s - 1, s, s + 1, NF - 1})
    wins = {0, 1, L.W - 2, L.W - 1}
    signed = L.widths[:-1]
    for j in range(1, len(signed)):
        if signed[j] != signed[j - 1]:
            wins |= {j - 1, j}
    return gens, sorted(wins)
