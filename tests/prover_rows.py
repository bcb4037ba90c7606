"""Chosen inputs for the batched prover's scalar stage (csrc/prover_batch.hpp: k_pb_init, k_pb_round, k_pb_final) and two
restatements of what it must leave behind, in big integers.  Nothing here imports the product.

A row names a curve, a shape (n, m), amounts, gammas, a challenge block [y, z, e, e_1..e_k] (None: the reference's literals),
blinding scalars [alpha, r, s, delta, eta, d_L[0..k), d_R[0..k)] (None: the literals) and whether BPP_PROVE_AMOUNT64 is set.
Every input is canonical; y and every e_t are non-zero (the whole kernels invert them), z and e may be zero.

Both models return (points, triple): `points` lists the 2k + 3 + m group elements of a proof in the numbering of pb_num_vps
-- 0 range A ; 1 + 2t L_t ; 2 + 2t R_t ; 2k + 1 wip.A ; 2k + 2 wip.B ; 2k + 3 + j V_j -- each as its coefficient map
{f: c != 0} over the fixed generators f = 0 g, 1 h, 2 + i G_i, 2 + mn + i H_i; `triple` is [r', s', delta'].
vps_wire() places a proof's maps where the kernels store them (fixed_term_index).  ONE difference, stated once: the H
coefficients of range A are -1, and k_pb_init stores them as +1 (k_fixed_msm negates the table entries of that virtual
proof instead); vps_wire flips them, the points keep the true -1.

  model_a   the reference's direction: src/range/mod.rs:80-187 / :240-403 and src/weighted_inner_product_proof.rs:36-227
            line by line over the group of coefficient maps -- the generator vectors ARE folded every round
            (wip.rs:151-163) and L, R, A, B are MulVecs over the folded vectors.  A folded generator has support
            {j = i mod n_t}, so a round costs O(mn).  d_L, d_R are the row's per-round scalars.
  model_b   the closed forms of the comment at the top of prover_batch.hpp, index by index: nothing but scalars is folded,
            cG_j / cH_j are products over the most significant bits of j.  fault= names ONE perturbation (FAULTS): the CPU
            test shows that each of them changes an output of the corpus wherever it can, i.e. that the rows discriminate.
"""

import functools
import random

import numpy as np

import recover_rows as RR
from recover_cases import ORDER

CURVES = RR.CURVES
KS = RR.KS
CAPPED_FROM_K = 9       # from here on a proof's arrays are megabytes (24 MB at k = 12): three rows per shape
FAULTS = ("halves_swapped", "y_power_sign", "dR_slot", "pz_m1", "e_swap_b", "amount_i32", "alpha_no_y")


def fixed_term_index(k, f):
    """MulVec order: head (3), g, h, L (k), R (k), G (mn), H (mn), V (m)"""
    return 3 + f if f < 2 else 5 + 2 * k + (f - 2)


def n_scalars(n, m):
    return 2 * n * m + 2 * RR.log2(n * m) + m + 5


def num_vps(k, m):
    return 2 * k + 3 + m


def literal_challenges(n, m):
    """range/mod.rs:109-110 / :278-279, wip.rs:131, :211"""
    return ([7, 7] if m == 1 else [12, 23]) + [99] + [7] * RR.log2(n * m)


def literal_blinding(n, m):
    """range/mod.rs:94 / :256, wip.rs:175-178, :94-95"""
    k = RR.log2(n * m)
    return [7 if m == 1 else 33, 33, 44, 88, 123] + [4] * k + [5] * k


def i32(v):
    """Rust `v as i32` (range/prover.rs:37)"""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


# ---- rows ----------------------------------------------------------------------------------------------------------------
class Row:
    """cname, n, m, k, name, flag (BPP_PROVE_AMOUNT64), values [m], gammas [m], ch [3 + k] or None, blind [5 + 2k] or None"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "<%s (%d,%d) %s>" % (self.cname, self.n, self.m, self.name)

    @property
    def r(self):
        return ORDER[self.cname]

    def ch_values(self):
        return literal_challenges(self.n, self.m) if self.ch is None else self.ch

    def blind_values(self):
        return literal_blinding(self.n, self.m) if self.blind is None else self.blind


def row_names(n, m):
    k = RR.log2(n * m)
    if k >= CAPPED_FROM_K:
        return ["random", "edges", "zero_a(z=1)"]
    return (["random", "ch(1)", "ch(-1)"] + ["top(%d)" % i for i in range(RR.TOP_VALUES)] +
            ["zero_a(z=0)", "zero_a(z=1)", "e_zero", "amount(0)", "amount(1)", "amount(max)", "amount(half)",
             "amount64(2^63)", "amount64(max)", "amount_i32_negative", "gamma(0)", "gamma(1)", "gamma(-1)", "identity",
             "blind(literal)", "blind_edges(0)", "blind_edges(1)", "blind_edges(2)", "blind(zero)", "literal"])


def make_row(cname, n, m, name):
    """the named row of a shape: what the name does not pin is drawn from a generator seeded by the arguments.
    top(i): [y, z, e, e_1..] = top[i], top[i + 1], ..: over i = 0..9 every limb-boundary value lands on y, on z, on e and on
    every e_t.  zero_a: a = -z (bit 0) or 1 - z (bit 1) is the zero vector, so c_L = c_R = 0 and r' = r.
    amount64(..): the flag set -- at n = 64 the amounts 2^63 and 2^64 - 1 of a real proof; below, the same words, of which
    the vectors read the low n bits and the commitment all 64.  edges (k >= 9): top(0), 2^64 - 1 with the flag, gammas
    0 / 1 / r - 1 and blind_edges(0) in one row."""
    r, k = ORDER[cname], RR.log2(n * m)
    if name not in row_names(n, m):
        raise ValueError("no row %r at (%d,%d)" % (name, n, m))
    rng = random.Random("prover rows/%s/%d/%d/%s" % (cname, n, m, name))
    nz = lambda: rng.randrange(1, r)
    ch = [nz() for _ in range(3 + k)]
    values = [rng.randrange(1 << n) for _ in range(m)]
    gammas = [rng.randrange(r) for _ in range(m)]
    blind = [rng.randrange(r) for _ in range(5 + 2 * k)]
    flag = False
    top = RR.top_values(r)
    edges3 = lambda i, cnt: [(0, 1, r - 1)[(s + i) % 3] for s in range(cnt)]
    if name == "ch(1)":
        ch = [1] * (3 + k)
    elif name == "ch(-1)":
        ch = [r - 1] * (3 + k)
    elif name.startswith("top("):
        i = int(name[4:-1])
        ch = [top[(i + s) % RR.TOP_VALUES] for s in range(3 + k)]
    elif name == "zero_a(z=0)":
        ch[1], values = 0, [0] * m
    elif name == "zero_a(z=1)":
        ch[1], values = 1, [(1 << n) - 1] * m
    elif name == "e_zero":
        ch[2] = 0
    elif name.startswith("amount("):
        v = {"0": 0, "1": 1, "max": (1 << n) - 1, "half": 1 << (n - 1)}[name[7:-1]]
        values = [v] * m
    elif name.startswith("amount64("):
        values, flag = [{"2^63": 1 << 63, "max": (1 << 64) - 1}[name[9:-1]]] * m, True
    elif name == "amount_i32_negative":
        values = [rng.getrandbits(64) | 0x80000000 for _ in range(m)]
        assert all(i32(v) < 0 for v in values)
    elif name.startswith("gamma("):
        gammas = [int(name[6:-1]) % r] * m
    elif name == "identity":
        values, gammas = [0] * m, [0] * m
    elif name == "blind(literal)":
        blind = None
    elif name.startswith("blind_edges("):
        blind = edges3(int(name[12:-1]), 5 + 2 * k)
    elif name == "blind(zero)":
        blind = [0] * (5 + 2 * k)
    elif name == "literal":
        ch = blind = None
    elif name == "edges":
        ch = [top[s % RR.TOP_VALUES] for s in range(3 + k)]
        values, flag, gammas, blind = [(1 << 64) - 1] * m, True, edges3(0, m), edges3(0, 5 + 2 * k)
    else:
        assert name == "random"
    return Row(cname=cname, n=n, m=m, k=k, name=name, flag=flag, values=values, gammas=gammas, ch=ch, blind=blind)


@functools.lru_cache(maxsize=None)
def shape_rows(cname, n, m):
    """every named row of one shape; made once, shared, never written to"""
    return tuple(make_row(cname, n, m, name) for name in row_names(n, m))


def corpus(cname, ks=KS):
    return [row for k in ks for n, m in RR.shapes(k) for row in shape_rows(cname, n, m)]


# ---- model A: the reference's direction over coefficient maps ----------------------------------------------------------------
def _mulvec(r, scalars, points):
    """MulVec::calculate over coefficient maps"""
    assert len(scalars) == len(points)
    out = {}
    for s, p in zip(scalars, points):
        if s:
            for f, c in p.items():
                out[f] = (out.get(f, 0) + s * c) % r
    return out


def _clean(p):
    return {f: c for f, c in p.items() if c}


def _amount_scalar(row, v, truncate=False):
    return v % row.r if row.flag and not truncate else i32(v) % row.r


def model_a(row):
    r, n, m, k = row.r, row.n, row.m, row.k
    mn = n * m
    inv = lambda x: pow(x, -1, r)
    y, z, e_final = row.ch_values()[:3]
    e_rounds = row.ch_values()[3:]
    bl = row.blind_values()
    alpha, rr, ss, delta, eta, d_Ls, d_Rs = bl[0], bl[1], bl[2], bl[3], bl[4], bl[5:5 + k], bl[5 + k:]
    g, h = {0: 1}, {1: 1}
    G = [{2 + i: 1} for i in range(mn)]
    H = [{2 + mn + i: 1} for i in range(mn)]
    # commitments                                                       range/prover.rs:34-40
    V = [_mulvec(r, [_amount_scalar(row, v), gm], [g, h]) for v, gm in zip(row.values, row.gammas)]
    # A = alpha h + sum (bit ? G_i : -H_i)                              range/mod.rs:94-107 / :256-277
    bits = [(row.values[i // n] >> (i % n)) & 1 for i in range(mn)]
    A = _mulvec(r, [alpha] + [1 if b else r - 1 for b in bits], [h] + [G[i] if b else H[i] for i, b in enumerate(bits)])
    power_of_two = [pow(2, i, r) for i in range(n)]
    power_of_y = [pow(y, i + 1, r) for i in range(mn)]
    power_of_y_rev = power_of_y[::-1]
    if m == 1:                                                          # range/mod.rs:125-172
        H_exp = [(power_of_two[i] * power_of_y_rev[i] + z) % r for i in range(n)]
        alpha_hat = (alpha + row.gammas[0] * pow(y, n + 1, r)) % r
    else:                                                               # range/mod.rs:290-376
        z_sqr = z * z % r
        power_of_z = [pow(z_sqr, j + 1, r) for j in range(m)]
        d = [e2 * ez % r for ez in power_of_z for e2 in power_of_two]
        H_exp = [(d[i] * power_of_y_rev[i] + z) % r for i in range(mn)]
        alpha_hat = (alpha + sum(pz * gm for pz, gm in zip(power_of_z, row.gammas)) * pow(y, mn + 1, r)) % r
    a = [(1 - z) % r if b else -z % r for b in bits]
    b = [H_exp[i] if bit else (H_exp[i] - 1) % r for i, bit in enumerate(bits)]
    # the argument                                                      wip.rs:36-227
    pw, alph, nn, Ls, Rs = power_of_y, alpha_hat, mn, [], []
    while nn != 1:
        t = len(Ls)
        nn //= 2
        a1, a2, b1, b2, y1, y2 = a[:nn], a[nn:], b[:nn], b[nn:], pw[:nn], pw[nn:]
        G1, G2, H1, H2 = G[:nn], G[nn:], H[:nn], H[nn:]
        c_L = sum(p * q * w for p, q, w in zip(a1, b2, y1)) % r
        c_R = sum(p * q * w for p, q, w in zip(a2, b1, y2)) % r
        y_nhat = y1[nn - 1]
        y_nhat_inv = inv(y_nhat)
        Ls.append(_mulvec(r, [y_nhat_inv * x % r for x in a1] + b2 + [c_L, d_Ls[t]], G2 + H1 + [g, h]))
        Rs.append(_mulvec(r, [y_nhat * x % r for x in a2] + b1 + [c_R, d_Rs[t]], G1 + H2 + [g, h]))
        e = e_rounds[t]
        e_inv = inv(e)
        a = [(a1[i] * e + a2[i] * y_nhat * e_inv) % r for i in range(nn)]
        b = [(b1[i] * e_inv + b2[i] * e) % r for i in range(nn)]
        G = [_mulvec(r, [e_inv, y_nhat_inv * e % r], [G1[i], G2[i]]) for i in range(nn)]      # wip.rs:151-163
        H = [_mulvec(r, [e, e_inv], [H1[i], H2[i]]) for i in range(nn)]
        pw = y1
        alph = (alph + e * e * d_Ls[t] + e_inv * e_inv * d_Rs[t]) % r
    rcbsca = (rr * pw[0] * b[0] + ss * pw[0] * a[0]) % r
    wA = _mulvec(r, [rr, ss, rcbsca, delta], [G[0], H[0], g, h])
    wB = _mulvec(r, [rr * pw[0] * ss % r, eta], [g, h])
    triple = [(rr + a[0] * e_final) % r, (ss + b[0] * e_final) % r, (eta + delta * e_final + alph * e_final * e_final) % r]
    points = [A] + [p for LR in zip(Ls, Rs) for p in LR] + [wA, wB] + V
    return [_clean(p) for p in points], triple


@functools.lru_cache(maxsize=None)
def expected(cname, n, m, name):
    """model A of a named row, computed once"""
    return model_a(make_row(cname, n, m, name))


# ---- model B: the closed forms of prover_batch.hpp --------------------------------------------------------------------------------
def model_b(row, fault=None):
    assert fault is None or fault in FAULTS
    r, n, m, k = row.r, row.n, row.m, row.k
    mn = n * m
    inv = lambda x: pow(x, -1, r)
    y, z, e_final = row.ch_values()[:3]
    et = row.ch_values()[3:]
    bl = row.blind_values()
    alpha, rr, ss, delta, eta = bl[:5]
    d_L = lambda t: bl[5 + t]
    d_R = lambda t: bl[5 + t] if fault == "dR_slot" else bl[5 + k + t]
    yinv, einv = inv(y), [inv(x) for x in et]
    msb = lambda j, t: (j >> (k - 1 - t)) & 1           # the t-th most significant bit of j
    gi, hi_ = lambda j: 2 + j, lambda j: 2 + mn + j
    bit = lambda i: (row.values[i // n] >> (i % n)) & 1
    A = {1: alpha}
    for i in range(mn):
        A[gi(i) if bit(i) else hi_(i)] = 1 if bit(i) else r - 1
    V = [{0: _amount_scalar(row, v, truncate=fault == "amount_i32"), 1: gm} for v, gm in zip(row.values, row.gammas)]
    pz = [1 if m == 1 else pow(z, 2 * (j + 1), r) for j in range(m)]
    d_of = lambda i: pow(2, i % n, r) * (1 if m == 1 else pz[i // n]) % r
    if fault == "pz_m1" and m == 1:
        pz = [z * z % r]
    a = [(1 - z) % r if bit(i) else -z % r for i in range(mn)]
    b = [(d_of(i) * pow(y, mn - i, r) + z - (0 if bit(i) else 1)) % r for i in range(mn)]
    alph = (alpha + (1 if fault == "alpha_no_y" else pow(y, mn + 1, r)) * sum(p * gm for p, gm in zip(pz, row.gammas))) % r
    cG, cH = [1] * mn, [1] * mn
    points = [A]
    for t in range(k):
        nt = mn >> t
        nh = nt >> 1
        yh = pow(y, nh, r)
        yhinv = yh if fault == "y_power_sign" else pow(yinv, nh, r)
        L = {0: sum(a[i] * b[nh + i] * pow(y, i + 1, r) for i in range(nh)) % r, 1: d_L(t)}
        R = {0: sum(a[nh + i] * b[i] * pow(y, nh + i + 1, r) for i in range(nh)) % r, 1: d_R(t)}
        for j in range(mn):
            i = j % nt
            if msb(j, t):       # G_j is in G2 (L, y^-n' a1), H_j in H2 (R, b1)
                L[gi(j)] = yhinv * a[i - nh] * cG[j] % r
                R[hi_(j)] = b[i - nh] * cH[j] % r
            else:               # G_j is in G1 (R, y^n' a2), H_j in H1 (L, b2)
                R[gi(j)] = yh * a[nh + i] * cG[j] % r
                L[hi_(j)] = b[nh + i] * cH[j] % r
        points += [L, R]
        e, ei = et[t], einv[t]
        for j in range(mn):
            hi = msb(j, t) ^ (1 if fault == "halves_swapped" else 0)
            cG[j] = cG[j] * (yhinv * e if hi else ei) % r
            cH[j] = cH[j] * (ei if hi else e) % r
        eb1, eb2 = (e, ei) if fault == "e_swap_b" else (ei, e)
        a = [(a[i] * e + a[nh + i] * yh * ei) % r for i in range(nh)]
        b = [(b[i] * eb1 + b[nh + i] * eb2) % r for i in range(nh)]
        alph = (alph + e * e * d_L(t) + ei * ei * d_R(t)) % r
    wA = {0: (rr * y * b[0] + ss * y * a[0]) % r, 1: delta}
    for j in range(mn):
        wA[gi(j)] = rr * cG[j] % r
        wA[hi_(j)] = ss * cH[j] % r
    points += [wA, {0: rr * y * ss % r, 1: eta}] + V
    triple = [(rr + a[0] * e_final) % r, (ss + b[0] * e_final) % r, (eta + delta * e_final + alph * e_final * e_final) % r]
    return [_clean(p) for p in points], triple


# ---- wire ------------------------------------------------------------------------------------------------------------------
def to_wire(xs):
    """ints < 2^256 -> (len, 4) uint64, little-endian words"""
    xs = list(xs)
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(len(xs), 4).copy()


def vps_wire(row, points):
    """(2k + 3 + m, N, 4) uint64: the scalar arrays as the kernels leave them -- range A's H terms as +1"""
    k, mn = row.k, row.n * row.m
    out = np.zeros((num_vps(k, row.m), n_scalars(row.n, row.m), 4), dtype=np.uint64)
    assert len(points) == out.shape[0]
    for v, p in enumerate(points):
        items = sorted(p.items())
        if items:
            vals = [(-c) % row.r if v == 0 and f >= 2 + mn else c for f, c in items]
            out[v, [fixed_term_index(k, f) for f, _ in items]] = to_wire(vals)
    return out
