"""One adversarial corpus for every verify entry point, with the verdict the DEFINITION gives each case.

The definition is the full-curve MulVec of RangeProof::verify: the C oracle (oracle/) on BLS12-381 and secp256k1, the
big-integer restatement (oracle/pyref.py, identity modulo E[4]) on edwards25519.  Nothing here imports the product.

corpus(cname, n, m, transcript=False) -> Corpus with .cases, a list of Case:
  pts (3 + 2k', PW) u64 [A, wip.A, wip.B, L.., R..]   sc (3, 4) u64 words as fed to the engine (possibly >= r)
  V (m, PW) u64      expect: definition verdict (0 Ok / 1 VerificationError)
  enc_ok: every point on the curve with canonical coordinates and k' = k      in_group: ... and in the prime-order group
  shifted: a point outside the prime-order group (BLS12-381 G1, or edwards25519 torsion)
  mv_scalars / result: the oracle's MulVec scalars (MulVec order) and result point for enc_ok cases
  status: the container status pyref.decode_proof assigns (0 / 1 / 2), None where the case has no compressed encoding
"""

import copy
import functools

import numpy as np

import oracle as O
import pyref as P

CID = {"bls12_381": 0, "secp256k1": 1, "ed25519": 2}
SHAPES = [(8, 1), (8, 2), (4, 4)]
BIG = (64, 16)
BIG_CASES = ("valid_1", "flip_s", "move_L0")
M256 = (1 << 256) - 1


class FastEdwards(P.EdwardsGroup):
    """pyref's EdwardsGroup with the scalar multiplication in extended coordinates (one inversion per product): the same
    group law, fast enough to prove and verify a few dozen edwards25519 proofs in a test"""

    def _ext(self, Pt):
        x, y = (0, 1) if Pt is None else Pt
        return (x, y, 1, x * y % self.p)

    def _add_ext(self, a, b):
        p, d2 = self.p, 2 * self.d
        X1, Y1, Z1, T1 = a
        X2, Y2, Z2, T2 = b
        A = (Y1 - X1) * (Y2 - X2) % p
        B = (Y1 + X1) * (Y2 + X2) % p
        C = T1 * d2 % p * T2 % p
        D = 2 * Z1 * Z2 % p
        E, F, G, H = B - A, D - C, D + C, B + A
        return (E * F % p, G * H % p, F * G % p, E * H % p)

    def _aff(self, e):
        X, Y, Z, _ = e
        zi = pow(Z, -1, self.p)
        x, y = X * zi % self.p, Y * zi % self.p
        return None if (x == 0 and y == 1) else (x, y)

    def mul(self, Pt, k):
        acc, q = self._ext(None), self._ext(Pt)
        while k:
            if k & 1:
                acc = self._add_ext(acc, q)
            q = self._add_ext(q, q)
            k >>= 1
        return self._aff(acc)

    def msm(self, scalars, points):
        acc = self._ext(None)
        for s, pt in zip(scalars, points):
            q = self._ext(pt)
            while s:
                if s & 1:
                    acc = self._add_ext(acc, q)
                q = self._add_ext(q, q)
                s >>= 1
        return self._aff(acc)


class Case:
    def __init__(self, name, pts, sc, V, **kw):
        self.name, self.pts, self.sc, self.V = name, pts, sc, V
        self.enc_ok, self.in_group, self.shifted, self.k_ok = True, True, False, True
        self.expect, self.mv_scalars, self.result, self.status = None, None, None, None
        self.sc_red = None          # the reduced scalars (the definition's values)
        self.t8 = False             # edwards25519: shifted by a point of order 8 (no ristretto255 encoding)
        self.__dict__.update(kw)

    def __repr__(self):
        return "Case(%s, expect=%s)" % (self.name, self.expect)


class Corpus:
    def __init__(self, cname, n, m, transcript):
        self.cname, self.cid, self.n, self.m, self.transcript = cname, CID[cname], n, m, transcript
        self.curve = P.CURVES[cname]
        self.r, self.p = self.curve["r"], self.curve["p"]
        self.mn = n * m
        self.k = self.mn.bit_length() - 1
        self.L = O.fp_limbs(self.cid)
        self.PW = 2 * self.L + 1
        if cname == "ed25519":
            self.grp = FastEdwards(self.curve)
            self.ppk = P.PublicKey(self.grp, self.mn)
            self.gh = O.points_to_wire(2, [self.ppk.g, self.ppk.h])
            self.G = O.points_to_wire(2, self.ppk.G_vec)
            self.H = O.points_to_wire(2, self.ppk.H_vec)
        else:
            self.grp = P.WeierstrassGroup(self.curve)
            self.opk = O.PublicKey(self.cid, self.mn)
            self.gh, self.G, self.H = self.opk.gh, self.opk.G, self.opk.H
        self.cases = []

    def by_name(self, name):
        return next(c for c in self.cases if c.name == name)

    # ---- the definition ----
    def key(self, perm=None):
        """the oracle's public key (C oracle or pyref), with G_vec permuted by perm: another key of the same shape"""
        if self.cname != "ed25519":
            if perm is None:
                return self.opk
            opk = O.PublicKey(self.cid, self.mn)
            opk.G = np.ascontiguousarray(self.G[perm])
            return opk
        if perm is None:
            return self.ppk
        ppk = copy.copy(self.ppk)
        ppk.G_vec = [self.ppk.G_vec[i] for i in perm]
        return ppk

    def commit(self, v, gamma):
        """RangeProver::commit: v as i32, gamma reduced mod r"""
        if self.cname != "ed25519":
            return O.commit(self.opk, v, gamma % self.r)
        pr = P.RangeProver()
        pr.commit(self.ppk, v, gamma % self.r)
        return O.point_to_wire(2, pr.commitment_vec[0])

    def prove(self, vals, gams, perm=None, V=None):
        """RangeProof::prove under key(perm); V: commitments to prove against instead of those of (v, gamma)"""
        gams = [g % self.r for g in gams]
        pk = self.key(perm)
        if self.cname != "ed25519":
            return O.range_prove(pk, self.n, vals, gams, V=V)
        pr = P.RangeProver()
        for v, g in zip(vals, gams):
            pr.commit(pk, v, g)
        if V is not None:
            pr.commitment_vec = O.wire_to_points(2, V)
        pf = P.RangeProof.prove(pk, self.n, pr)
        w = pf.proof
        pts = O.points_to_wire(2, [pf.A, w.A, w.B] + list(w.L_vec) + list(w.R_vec))
        return pts, O.scalars_to_wire([w.r_prime, w.s_prime, w.d_prime]), O.points_to_wire(2, pr.commitment_vec)

    def verdict(self, pts, sc, V, perm=None):
        """the definition verdict of a record with a valid encoding under key(perm) (scalars reduced, infinity canonical)"""
        red = [O.limbs_to_int(sc[i]) % self.r for i in range(3)]
        pts = canonical_inf(self, pts)
        if self.cname != "ed25519":
            return int(O.range_verify(self.key(perm), self.n, self.m, pts, O.scalars_to_wire(red), V))
        pp = O.wire_to_points(2, pts)
        k = self.k
        pf = P.RangeProof(pp[0], P.WeightedInnerProductProof(pp[3:3 + k], pp[3 + k:3 + 2 * k], pp[1], pp[2], *red))
        mv = pf.verify_mulvec(self.key(perm), self.n, O.wire_to_points(2, V))
        if mv is None:
            return 1
        return 0 if self.grp.is_identity_class(self.grp.msm(mv.scalars, mv.points)) else 1

    def judge(self, c):
        """fills c.expect (and mv_scalars / result for a valid encoding)"""
        red = [O.limbs_to_int(c.sc[i]) % self.r for i in range(3)]
        c.sc_red = O.scalars_to_wire(red)
        if not c.enc_ok or not c.k_ok:
            c.expect = 1
            return
        pts = canonical_inf(self, c.pts)
        if self.cname != "ed25519":
            rc, vsc, res = O.range_verify(self.opk, self.n, self.m, pts, c.sc_red, c.V, want_scalars=True,
                                          want_result=True)
            c.expect = int(rc)
            c.mv_scalars = O.wire_to_scalars(vsc)
            c.result = O.wire_to_point(self.cid, res)
            return
        pp = O.wire_to_points(2, pts)
        k = self.k
        pf = P.RangeProof(pp[0], P.WeightedInnerProductProof(pp[3:3 + k], pp[3 + k:3 + 2 * k], pp[1], pp[2], *red))
        mv = pf.verify_mulvec(self.ppk, self.n, O.wire_to_points(2, c.V))
        if mv is None:
            c.expect = 1
            return
        c.mv_scalars = list(mv.scalars)
        c.result = self.grp.msm(mv.scalars, mv.points)
        c.expect = 0 if self.grp.is_identity_class(c.result) else 1

    def scalar_index(self, rec_idx):
        """MulVec index of record point rec_idx ([A, wip.A, wip.B, L.., R.., V..]): range/mod.rs:492-494 for m > 1,
        wip.rs:309-311 (B, A', A) for m = 1"""
        k, mn = self.k, self.mn
        if rec_idx < 3:
            return rec_idx if self.m > 1 else 2 - rec_idx
        if rec_idx < 3 + 2 * k:
            return 5 + (rec_idx - 3)
        return 5 + 2 * k + 2 * mn + (rec_idx - 3 - 2 * k)

    def container_status(self, c):
        """status of pyref.decode_proof on the compressed encoding (FormatError = 2), else the verdict"""
        if not c.enc_ok or c.t8 or not c.k_ok:     # no encoding, or one of another length
            return None
        grp = self.grp
        for w in c.pts:
            if not P.point_in_prime_subgroup(self.curve, grp, O.wire_to_point(self.cid, w) if not w[2 * self.L] else None):
                return 2
        if any(O.limbs_to_int(c.sc[i]) >= self.r for i in range(3)):
            return 2
        return c.expect


def canonical_inf(cp, pts):
    """any non-zero flag word is infinity: the definition's point is the canonical one"""
    pts = pts.copy()
    for i in range(pts.shape[0]):
        if pts[i, 2 * cp.L]:
            pts[i] = 0
            pts[i, 2 * cp.L] = 1
    return pts


def _wire(cp, Pt):
    return O.point_to_wire(cp.cid, Pt)


def _pt(cp, w):
    return O.wire_to_point(cp.cid, w)


def bls_T():
    """T = (0, 2): on y^2 = x^3 + 4, of order 3"""
    return (0, 2)


def ed_torsion(order):
    """an edwards25519 point of exact order 4 or 8"""
    c = P.ED25519
    p, d = c["p"], c["d"]
    if order == 4:
        return (pow(2, (p - 1) // 4, p), 0)
    G = FastEdwards(c)
    y = 2
    while True:
        u, v = (y * y - 1) % p, (d * y * y + 1) % p
        ok, x = P.Ristretto255.sqrt_ratio_m1(u, v)
        if ok:
            T = G.mul((x, y), c["r"])          # in E[8]
            if T is not None and G.mul(T, 4) is not None:
                return T
        y += 1


def _add_cases(cp, base, names=None):
    """the tampered / edge cases derived from the valid proof `base` (pts, sc, V)"""
    pts0, sc0, V0 = base
    k, L, PW, r, cid = cp.k, cp.L, cp.PW, cp.r, cp.cid
    grp = cp.grp
    g = _pt(cp, cp.gh[0])
    out = []

    def add(name, pts=None, sc=None, V=None, **kw):
        if names is not None and name not in names:
            return
        out.append(Case(name, pts0.copy() if pts is None else pts, sc0.copy() if sc is None else sc,
                        V0.copy() if V is None else V, **kw))

    # scalars: one flipped bit each; non-canonical r' + r and r' + j r
    for t, nm in enumerate(("r", "s", "d")):
        s = sc0.copy()
        s[t, 0] ^= np.uint64(1)
        add("flip_" + nm, sc=s)
    r0 = O.limbs_to_int(sc0[0])
    j = (M256 - r0) // r
    if j >= 1:
        s = sc0.copy()
        s[0] = O.int_to_limbs(r0 + r, 4)
        add("nc_r_plus_r", sc=s)
    if j >= 2:
        s = sc0.copy()
        s[0] = O.int_to_limbs(r0 + j * r, 4)
        add("nc_r_plus_%dr" % j, sc=s, j=j)

    def moved(idx, delta, name, **kw):
        p = pts0.copy()
        p[idx] = _wire(cp, grp.add(_pt(cp, pts0[idx]), delta))
        add(name, pts=p, **kw)

    moved(0, g, "move_A")
    moved(1, g, "move_wA")
    moved(2, g, "move_wB")
    moved(3, g, "move_L0")
    moved(3 + 2 * k - 1, g, "move_Rlast")
    V = V0.copy()
    V[-1] = _wire(cp, grp.add(_pt(cp, V0[-1]), g))
    add("move_Vlast", V=V)
    V = V0.copy()
    V[-1] = _wire(cp, grp.neg(_pt(cp, V0[-1])))
    add("neg_Vlast", V=V)
    # special sums
    p = pts0.copy()
    p[3] = pts0[3 + k]
    add("L0_eq_R0", pts=p)
    p = pts0.copy()
    p[3] = _wire(cp, grp.neg(_pt(cp, pts0[3 + k])))
    add("L0_neg_R0", pts=p)
    p = pts0.copy()
    p[0] = cp.G[0]
    add("A_eq_G0", pts=p)
    p = pts0.copy()
    p[3] = 0
    p[3, 2 * L] = 1
    add("L0_inf", pts=p)
    p = pts0.copy()
    p[3] = pts0[4 if k > 1 else 3 + k]
    p[3, 2 * L] = 5
    add("L0_inf_flag5", pts=p)
    # invalid encodings
    p = pts0.copy()
    for bit in (1, 2, 4):
        p[1] = pts0[1]
        p[1, L] ^= np.uint64(bit)
        if not grp.on_curve(_pt(cp, p[1])):
            break
    add("off_curve_wA", pts=p, enc_ok=False, in_group=False)
    x = O.limbs_to_int(pts0[3, :L])
    if x + cp.p < (1 << (64 * L)):
        p = pts0.copy()
        p[3, :L] = O.int_to_limbs(x + cp.p, L)
        add("L0_x_plus_p", pts=p, enc_ok=False, in_group=False)
    p = np.concatenate([pts0[:3 + k - 1], pts0[3 + k:3 + 2 * k - 1]])
    add("wrong_k", pts=p, k_ok=False, in_group=False)
    return out


def _curve_specific(cp, base, names=None):
    pts0, sc0, V0 = base
    k = cp.k
    grp = cp.grp
    out = []

    def add(name, pts, **kw):
        if names is None or name in names:
            out.append(Case(name, pts, sc0.copy(), V0.copy(), **kw))

    if cp.cname == "bls12_381":
        T = bls_T()
        p = pts0.copy()
        p[3 + k] = _wire(cp, grp.add(_pt(cp, pts0[3 + k]), T))
        add("R0_plus_T", p, in_group=False, shifted=True)
        p = pts0.copy()
        p[0] = _wire(cp, T)
        add("A_eq_T", p, in_group=False, shifted=True)
        # the cancelling pair: T on point i, c T on point j with s_i + c s_j = 0 (mod 3) -- the full-curve sum is unchanged
        _, vsc, _ = O.range_verify(cp.opk, cp.n, cp.m, pts0, sc0, V0, want_scalars=True)
        s = O.wire_to_scalars(vsc)
        cand = list(range(3 + 2 * k))
        for i in cand:
            for j in cand:
                si, sj = s[cp.scalar_index(i)] % 3, s[cp.scalar_index(j)] % 3
                if i < j and si and sj:
                    c = (-si * pow(sj, -1, 3)) % 3
                    p = pts0.copy()
                    p[i] = _wire(cp, grp.add(_pt(cp, pts0[i]), T))
                    cT = T if c == 1 else grp.neg(T)    # not grp.mul: the reference's doubling maps x = 0 to O
                    p[j] = _wire(cp, grp.add(_pt(cp, pts0[j]), cT))
                    add("cancel_pair", p, in_group=False, shifted=True, pair=(i, j, c))
                    break
            else:
                continue
            break
    if cp.cname == "ed25519":
        T4, T8 = ed_torsion(4), ed_torsion(8)
        p = pts0.copy()
        p[0] = _wire(cp, grp.add(_pt(cp, pts0[0]), T4))
        add("A_plus_T4", p, in_group=False, shifted=True)
        pv = cp.by_name("valid_1").mv_scalars
        for want, nm in ((0, "T8_even"), (1, "T8_odd")):
            for i in range(3 + 2 * k + cp.m):       # proof points first, then the commitments
                if pv[cp.scalar_index(i)] % 2 == want:
                    p, V = pts0.copy(), V0.copy()
                    if i < 3 + 2 * k:
                        p[i] = _wire(cp, grp.add(_pt(cp, pts0[i]), T8))
                    else:
                        V[i - 3 - 2 * k] = _wire(cp, grp.add(_pt(cp, V0[i - 3 - 2 * k]), T8))
                    if names is None or nm in names:
                        out.append(Case(nm, p, sc0.copy(), V, in_group=False, shifted=True, t8=True, moved_idx=i))
                    break
    return out


@functools.lru_cache(maxsize=None)
def corpus(cname, n, m, transcript=False):
    """the corpus of one (curve, n, m); transcript=True: the valid and scalar-tamper cases under the Fiat-Shamir
    transcript (BLS12-381 and secp256k1: the C oracle's transcript mode)"""
    cp = Corpus(cname, n, m, transcript)
    r = cp.r
    big = (n, m) == BIG
    if transcript:
        assert cname != "ed25519"
        O.set_transcript(True)
    try:
        def vg(v, g):
            return [v] + [(v * 7 + i) % (1 << n) for i in range(1, m)], [g] + [g + 3 * i for i in range(1, m)]

        wit = [("valid_1", *vg(200 % (1 << n), 3)), ("valid_2", *vg(5, 11))]
        if not big and not transcript:
            wit += [("v_zero", *vg(0, 7)), ("v_max", *vg((1 << n) - 1, 7)), ("gamma_zero", *vg(9, 0)),
                    ("gamma_rm1", *vg(9, r - 1)), ("v_2n", *vg(1 << n, 5)), ("v_wrap31", *vg((1 << 31) + 5, 5)),
                    ("v_wrap40", *vg((1 << 40) + 3, 5))]
        proofs = {}
        for name, vals, gams in wit:
            if big and name != "valid_1":
                continue
            proofs[name] = cp.prove(vals, gams)
            cp.cases.append(Case(name, *proofs[name], witness=(vals, gams)))
        base = proofs["valid_1"]
        names = BIG_CASES if big else None
        if transcript:
            names = ("flip_r", "flip_s", "flip_d", "nc_r_plus_r")
        cp.cases += _add_cases(cp, base, names)
        for c in cp.cases:
            cp.judge(c)
        if not transcript and not big:
            extra = _curve_specific(cp, base)
            for c in extra:
                cp.judge(c)
            cp.cases += extra
        if big:
            cp.cases = [c for c in cp.cases if c.name in BIG_CASES]
        if not transcript:
            for c in cp.cases:
                c.status = cp.container_status(c)
    finally:
        if transcript:
            O.set_transcript(False)
    return cp


def encode_case(cp, c, version=1):
    """pyref's container encoding of case c and its compressed commitments: (proof bytes, commitments bytes)"""
    k = (c.pts.shape[0] - 3) // 2
    pp = O.wire_to_points(cp.cid, canonical_inf(cp, c.pts))
    sc = [O.limbs_to_int(c.sc[i]) for i in range(3)]
    pf = P.RangeProof(pp[0], P.WeightedInnerProductProof(pp[3:3 + k], pp[3 + k:3 + 2 * k], pp[1], pp[2], *sc))
    blob = P.encode_proof(cp.curve, cp.n, cp.m, pf, version)
    enc = P.compress_point if version == 1 else P.uncompressed_point
    comm = b"".join(enc(cp.curve, Vp) for Vp in O.wire_to_points(cp.cid, c.V))
    return blob, comm
