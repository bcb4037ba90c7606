"""Shared case builder of the WIP-seam tests (CPU: test_wip_abi_cpu.py, GPU: test_gpu_wip.py).  Nothing here imports the
product: the cases are built with oracle/pyref.py alone.

A case is one instance of the relation WeightedInnerProductProof proves (reference src/weighted_inner_product_proof.rs)
    P = sum a_i G_i + sum b_i H_i + (sum a_i b_i y^(i+1)) g + gamma h
together with a statement (Gc, Hc, gc, Vc, V) -- the four *_exp_of_commitment arguments of verify (wip.rs:238-247) and the
statement points -- and the A' that makes the statement true:
    A' = P - sum Gc_i G_i - sum Hc_i H_i - gc g - sum Vc_j V_j
so that verify_mulvec(pk, [y^(i+1)], Gc, Hc, gc, Vc, A', V) of a proof for (a, b, y, gamma) sums to the identity.

range_exponents restates the exponents the range statement hands to that seam: src/range/mod.rs:189-238 (m = 1) and
:405-477 (m > 1).
"""

import random

import pyref as P


class WipCase:
    def __init__(self, pk, a, b, y, gamma, Gc, Hc, gc, Vc, V, A_prime):
        self.pk, self.a, self.b, self.y, self.gamma = pk, a, b, y, gamma
        self.Gc, self.Hc, self.gc, self.Vc, self.V, self.A_prime = Gc, Hc, gc, Vc, V, A_prime

    @property
    def length(self):
        return len(self.a)

    @property
    def nv(self):
        return len(self.V)

    def powers(self):
        """power_of_y_vec = exp_iter_type2(y, len)"""
        return P.Fr(self.pk.G.r).exp_iter_type2(self.y % self.pk.G.r, self.length)

    def statement(self):
        """the seam's statement block [Gc (len), Hc (len), gc, Vc (nv)]"""
        return list(self.Gc) + list(self.Hc) + [self.gc] + list(self.Vc)

    def prove(self):
        """pyref's prover on this case (literal mode, or whatever pyref.Transcript is set to)"""
        r = self.pk.G.r
        return P.WeightedInnerProductProof.prove(self.pk, [x % r for x in self.a], [x % r for x in self.b], self.powers(),
                                                 self.gamma % r, None)

    def mulvec(self, proof, **tamper):
        """verify_mulvec of `proof` against this case's statement; tamper: A_prime= / V= / Gc= ... overrides"""
        g = dict(Gc=self.Gc, Hc=self.Hc, gc=self.gc, Vc=self.Vc, A_prime=self.A_prime, V=self.V)
        g.update(tamper)
        return proof.verify_mulvec(self.pk, self.powers(), g["Gc"], g["Hc"], g["gc"], g["Vc"], g["A_prime"], g["V"])


def commitment_P(pk, a, b, y, gamma):
    """the P of the relation"""
    G, r = pk.G, pk.G.r
    acc, c, yp = G.zero(), 0, 1
    for i in range(len(a)):
        yp = yp * y % r
        c = (c + a[i] * b[i] % r * yp) % r
        acc = G.add(acc, G.add(G.mul(pk.G_vec[i], a[i] % r), G.mul(pk.H_vec[i], b[i] % r)))
    return G.add(acc, G.add(G.mul(pk.g, c), G.mul(pk.h, gamma % r)))


def a_prime_for(pk, Pt, Gc, Hc, gc, Vc, V):
    G, r = pk.G, pk.G.r
    acc = Pt
    for i in range(len(Gc)):
        acc = G.add(acc, G.neg(G.add(G.mul(pk.G_vec[i], Gc[i] % r), G.mul(pk.H_vec[i], Hc[i] % r))))
    acc = G.add(acc, G.neg(G.mul(pk.g, gc % r)))
    for c, v in zip(Vc, V):
        acc = G.add(acc, G.neg(G.mul(v, c % r)))
    return acc


def random_case(pk, nv, seed, zero_ends=False, over_r=False):
    """random a, b, y, gamma and a random statement over pk (length = len(pk.G_vec)).  zero_ends: a[0] = a[-1] = 0.
    over_r: a[1 mod len], y and gamma are handed over as values >= r (the definition reduces them)."""
    rng = random.Random(seed)
    r = pk.G.r
    n = len(pk.G_vec)
    a = [rng.randrange(r) for _ in range(n)]
    b = [rng.randrange(r) for _ in range(n)]
    y, gamma = rng.randrange(1, r), rng.randrange(r)
    if zero_ends:
        a[0] = a[-1] = 0
    if over_r:   # small values, so that value + r still fits the 256-bit wire scalar on every curve
        a[1 % n], y, gamma = rng.randrange(1 << 64), rng.randrange(1, 1 << 64), rng.randrange(1 << 64)
    Gc = [rng.randrange(r) for _ in range(n)]
    Hc = [rng.randrange(r) for _ in range(n)]
    gc = rng.randrange(r)
    Vc = [rng.randrange(1, r) for _ in range(nv)]
    V = [pk.G.mul(pk.g, rng.randrange(1, r)) for _ in range(nv)]
    Ap = a_prime_for(pk, commitment_P(pk, a, b, y, gamma), Gc, Hc, gc, Vc, V)
    if over_r:
        a[1 % n], y, gamma = a[1 % n] + r, y + r, gamma + r
    return WipCase(pk, a, b, y, gamma, Gc, Hc, gc, Vc, V, Ap)


def range_exponents(r, n, m, y, z):
    """(Gc, Hc, gc, Vc) of the range statement for challenges y, z: range/mod.rs:189-238 (m = 1), :405-477 (m > 1)"""
    F = P.Fr(r)
    mn = n * m
    p2 = F.exp_iter_type1(2, n)
    py = F.exp_iter_type2(y, mn)
    y_mn1 = F.scalar_exp_vartime(y, mn + 1)
    Gc = [(-z) % r] * mn
    if m == 1:
        Hc = [(p2[i] * py[n - 1 - i] + z) % r for i in range(n)]
        gc = sum(py) % r * (z - z * z) % r
        gc = (gc - (F.scalar_exp_vartime(2, n) - 1) * y_mn1 * z) % r
        return Gc, Hc, gc, [y_mn1]
    zsq = z * z % r
    pz = F.exp_iter_type2(zsq, m)
    d = [e2 * ez % r for ez in pz for e2 in p2]
    Hc = [(d[i] * py[mn - 1 - i] + z) % r for i in range(mn)]
    gc = (F.sum_of_powers_type2(y, mn) * (z - zsq) - y_mn1 * z * F.sum_of_powers_type1(F.new(2), n)
          * F.sum_of_powers_type2(zsq, m)) % r
    return Gc, Hc, gc, [x * y_mn1 % r for x in pz]


def range_case(pk, n, values, gammas):
    """the range statement of (values, gammas) under pyref's literal challenges as a WipCase: a, b, alpha_hat from
    pyref's own prover (its trace), the exponents from range_exponents, A' = the range proof's A, V = the commitments.
    Returns (case, range proof)."""
    r = pk.G.r
    m = len(values)
    pr = P.RangeProver()
    for v, g in zip(values, gammas):
        pr.commit(pk, v, g % r)
    trace = []
    proof = P.RangeProof.prove(pk, n, pr, trace)
    t = next(x for x in trace if x.get("stage") == "range")
    y, z = P.Transcript.yz(m)
    Gc, Hc, gc, Vc = range_exponents(r, n, m, y, z)
    return WipCase(pk, t["a_vec"], t["b_vec"], y, t["alpha_hat"], Gc, Hc, gc, Vc, list(pr.commitment_vec), proof.A), proof


# the single-field tampers of the GPU tests: name -> (what it changes)
TAMPERS = ("A_prime", "wip_A", "L0", "R_last", "V0", "r_prime", "s_prime", "d_prime", "Gc_last", "Hc0", "gc", "Vc0")


def tampered(case, proof, name):
    """(proof', overrides for WipCase.mulvec) with the one field `name` changed"""
    G, r = case.pk.G, case.pk.G.r
    bump = lambda Pt: G.add(Pt, case.pk.g)
    q = P.WeightedInnerProductProof(list(proof.L_vec), list(proof.R_vec), proof.A, proof.B, proof.r_prime, proof.s_prime,
                                    proof.d_prime)
    ov = {}
    if name == "A_prime":
        ov["A_prime"] = bump(case.A_prime)
    elif name == "wip_A":
        q.A = bump(q.A)
    elif name == "L0":
        q.L_vec[0] = bump(q.L_vec[0])
    elif name == "R_last":
        q.R_vec[-1] = bump(q.R_vec[-1])
    elif name == "V0":
        ov["V"] = [bump(case.V[0])] + list(case.V[1:])
    elif name in ("r_prime", "s_prime", "d_prime"):
        setattr(q, name, (getattr(q, name) + 1) % r)
    elif name == "Gc_last":
        ov["Gc"] = list(case.Gc[:-1]) + [(case.Gc[-1] + 1) % r]
    elif name == "Hc0":
        ov["Hc"] = [(case.Hc[0] + 1) % r] + list(case.Hc[1:])
    elif name == "gc":
        ov["gc"] = (case.gc + 1) % r
    elif name == "Vc0":
        ov["Vc"] = [(case.Vc[0] + 1) % r] + list(case.Vc[1:])
    else:
        raise KeyError(name)
    return q, ov
