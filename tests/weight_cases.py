"""Shared case builder of the weight tests (CPU: test_weight_cases_cpu.py, GPU: test_gpu_weights.py): WHICH 128-bit weight
the combined and the grouped check (csrc/combined.hpp) give WHICH proof, pinned by batches of invalid proofs that pass under
exactly those weights.  Nothing here imports the product: hashlib, big integers, scalar_cases and oracle/pyref.py.

The definition (csrc/combined.hpp, comb_weight):
    w_p = SHA-256(key || "bppw" || (index_base + p) as u64 LE)[0..16)   read little-endian, 0 -> 1          (key form)
    w_p = the caller's 16 bytes of proof p                               read little-endian, 0 -> 1          (raw form)
with p the CALLER's position, also where the batch is gathered by aggregation size or cut over the shards of a pool.

The instrument: a defect that moves a valid proof's verification MulVec M_p along the generator h alone, M_p = x_p h with
x_p = coefficient * defect known in big integers.  A weighted check over a set of such proofs sees (sum_p w_p x_p) h, the
identity iff sum_p w_p x_p = 0 (mod r): every defect of a set but the last is drawn, the last is solved so that the sum
vanishes under the definition -- and then under no other weight rule (faults, below), which test_weight_cases_cpu.py shows
in big integers for every plan before test_gpu_weights.py asks the device.  Defect kinds:
    ("D", 0)   delta' <- delta' + d (mod r)     x = c_h d,  c_h the coefficient of delta' in h_exp (by differencing)
    ("A", j)   record point j <- it + t h       x = s t,    s the MulVec scalar of [A, wip.A, wip.B][j]
    ("V", j)   V_j <- V_j + t h                 x = V_exp[j] t
A and V need fixed challenges (the points are hashed by the transcript); D does not, delta' is drawn after the last one.
"""

import functools
import hashlib
import random

import pyref as P
import scalar_cases as SC

TAG = b"bppw"
M64 = (1 << 64) - 1

# the wrong rules a consistent-but-wrong device could follow; each leaves verdict parity with the exact path intact
FAULTS = ("one", "low64", "low32", "bytes16_32", "big_endian", "no_tag", "no_key", "index32", "no_base", "gathered",
          "shard_local")
RAW_FAULTS = ("zero_stays_zero",)


def weight(key, index, fault=None, index_base=0, gathered=None, shard_lo=0):
    """The weight of the proof with GLOBAL index `index` = index_base + caller position.  fault: one of FAULTS --
    one: every weight 1;  low64 / low32: only the low bits of the 128;  bytes16_32: the other half of the digest;
    big_endian: the 16 bytes read big-endian;  no_tag: "bppw" left out;  no_key: the key not read (32 zero bytes);
    index32: the high word of the index dropped;  no_base: index_base ignored;  gathered: the position in the batch
    gathered by aggregation size instead of the caller's;  shard_local: the shard's first proof `shard_lo` not added."""
    assert len(key) == 32 and 0 <= index < 1 << 64 and (fault is None or fault in FAULTS)
    if fault == "one":
        return 1
    if fault == "index32":
        index &= 0xFFFFFFFF
    elif fault == "no_base":
        index -= index_base
    elif fault == "gathered":
        index = index_base + gathered
    elif fault == "shard_local":
        index -= shard_lo
    if fault == "no_key":
        key = bytes(32)
    dg = hashlib.sha256(key + (b"" if fault == "no_tag" else TAG) + index.to_bytes(8, "little")).digest()
    w = int.from_bytes(dg[16:32] if fault == "bytes16_32" else dg[:16], "big" if fault == "big_endian" else "little")
    if fault == "low64":
        w &= M64
    elif fault == "low32":
        w &= 0xFFFFFFFF
    return w or 1


def raw_weight(bytes16, fault=None):
    """the weight a caller's 16 bytes stand for; fault zero_stays_zero: sixteen zero bytes weigh 0 instead of 1"""
    assert len(bytes16) == 16 and (fault is None or fault in RAW_FAULTS)
    w = int.from_bytes(bytes16, "little")
    return w if (w or fault == "zero_stays_zero") else 1


# ---- x_p per unit of defect, from the restatement ----------------------------------------------------------------------
def literal_challenges(n, m):
    """(y, z, e, [e_1..e_k]) of the reference's constants (pyref.Transcript)"""
    T = P.Transcript
    y, z = (T.Y_SINGLE, T.Z_SINGLE) if m == 1 else (T.Y_MULTI, T.Z_MULTI)
    return y, z, T.E_FINAL, [T.E_ROUND] * SC.log2(n * m)


def fs_challenges(curve, n, m, ppk, points, V):
    """(y, z, e, [e_1..e_k]) the transcript derives from a proof record: points = [A, wip.A, wip.B, L.., R..] and V as affine
    pairs (None = infinity), ppk the pyref public key of the shape"""
    k = SC.log2(n * m)
    wip = P.WeightedInnerProductProof(list(points[3:3 + k]), list(points[3 + k:3 + 2 * k]), points[1], points[2], 0, 0, 0)
    ch = P.FsTranscript(P.CURVES[curve], SC.CURVES.index(curve), n, m, ppk).verifier_challenges(P.RangeProof(points[0], wip), V)
    return ch["y"], ch["z"], ch["e"], list(ch["e_rounds"])


def coefficient(curve, n, m, kind, j=0, challenges=None):
    """x_p per unit of defect of kind (kind, j) for a proof of shape (n, m) under `challenges` (None: the literals)"""
    y, z, e, er = challenges if challenges is not None else literal_challenges(n, m)
    return _coefficient(curve, n, m, kind, j, y, z, e, tuple(er))


@functools.lru_cache(maxsize=None)
def _coefficient(curve, n, m, kind, j, y, z, e, er):
    r = SC.order(curve)
    er = list(er)
    k, mn = SC.log2(n * m), n * m
    base = SC.range_scalars_direct(curve, n, m, y, z, e, er, [0, 0, 0])
    if kind == "D":
        moved = SC.range_scalars_direct(curve, n, m, y, z, e, er, [0, 0, 1])
        assert [i for i in range(len(base)) if base[i] != moved[i]] == [4]     # delta' enters h's scalar and no other
        return (moved[4] - base[4]) % r
    if kind == "A":
        assert 0 <= j < 3
        return base[2 - j if m == 1 else j]      # the MulVec's head is [wip.B, wip.A, A] for m = 1, [A, wip.A, wip.B] beyond
    assert kind == "V" and 0 <= j < m
    return base[5 + 2 * k + 2 * mn + j]


def solve_last(weights, coeffs, defects, r):
    """the last defect of a set: sum_p w_p c_p d_p = 0 (mod r) with defects = those of all members but the last"""
    assert len(weights) == len(coeffs) == len(defects) + 1 >= 2
    acc = sum(w * c * d for w, c, d in zip(weights, coeffs, defects)) % r
    last = weights[-1] * coeffs[-1] % r
    assert last
    return -acc * pow(last, -1, r) % r


# ---- who sits where ------------------------------------------------------------------------------------------------------
def uniform_cuts(count, world):
    """the cut of a uniform batch: sizes differ by at most one, the larger shards first"""
    base, rem = divmod(count, world)
    return [rk * base + min(rk, rem) for rk in range(world)] + [count]


def cost_cuts(ms, world):
    """the cut of a batch whose proof i costs ms[i] (include/bpp_amd.h, "verifier pool"): shard rk starts at the first proof
    whose cost prefix reaches rk / world of the total"""
    total, out, rk, prefix = sum(ms), [0], 1, 0
    for i, m in enumerate(ms):
        while rk < world and world * prefix >= rk * total:
            out.append(i)
            rk += 1
        prefix += m
    return out + [len(ms)] * (world + 1 - len(out))


def gathered_order(ms, lo, hi):
    """the caller positions lo..hi-1 gathered by aggregation size: those with m = 1 in caller order, then 2, 4, ..."""
    return sorted(range(lo, hi), key=lambda p: ms[p])      # sorted() is stable


def pick(ms, distinct):
    """which of the `distinct` base proofs of its class caller position p replicates: the classes' own counters, cycling"""
    seen, out = {}, []
    for m in ms:
        out.append(seen.get(m, 0) % distinct)
        seen[m] = seen.get(m, 0) + 1
    return out


# ---- plans -------------------------------------------------------------------------------------------------------------
class Plan:
    """One batch for one entry: per caller position the shape m, the defect kind and the defect (0: the proof stays valid).

    group None: one weighted sum over the whole batch (the combined check, also over ranks and shards: they add up);
    else one sum per group of `group` neighbours of each shard's slice gathered by aggregation size.  cuts: the shards
    (a lone verifier: [0, count]).  raw: the caller's 16 bytes per proof instead of a key.  challenges[p]: None = literals.
    solved_under: the rule the last defect of every set was solved under (None = the definition; a fault = a control that
    the definition must reject)."""

    def __init__(self, name, curve, n, ms, kinds, sets, rng, key=None, index_base=0, raw=None, group=None, cuts=None,
                 challenges=None, solved_under=None):
        self.name, self.curve, self.n, self.ms, self.kinds = name, curve, n, list(ms), list(kinds)
        self.count = len(self.ms)
        self.key, self.index_base, self.raw, self.group = key, index_base, raw, group
        self.cuts = list(cuts) if cuts is not None else [0, self.count]
        self.challenges = list(challenges) if challenges is not None else [None] * self.count
        self.solved_under = solved_under
        self.r = SC.order(curve)
        assert (key is None) != (raw is None) and len(self.kinds) == self.count and self.index_base + self.count <= 1 << 64
        self.coeffs = [coefficient(curve, n, m, kd, j, ch) for m, (kd, j), ch in zip(self.ms, self.kinds, self.challenges)]
        assert all(self.coeffs)
        self.gathered, self.shard_lo, self.groups = [None] * self.count, [None] * self.count, []
        for lo, hi in zip(self.cuts, self.cuts[1:]):
            order = gathered_order(self.ms, lo, hi)
            for g, p in enumerate(order):
                self.gathered[p], self.shard_lo[p] = g, lo
            if group is not None:
                self.groups += [order[i:i + group] for i in range(0, len(order), group)]
        if group is None:
            self.groups = [list(range(self.count))]
        self.sets = [list(s) for s in sets]
        self.defects = [0] * self.count
        w = self.weights(solved_under)
        for s in self.sets:
            assert len(s) >= 2 and all(self.defects[p] == 0 for p in s)
            while True:
                ds = [rng.randrange(1, self.r) for _ in s[:-1]]
                last = solve_last([w[p] for p in s], [self.coeffs[p] for p in s], ds, self.r)
                if 0 < last < self.r:           # non-zero and canonical, else redraw
                    break
            for p, d in zip(s, ds + [last]):
                self.defects[p] = d

    def weights(self, fault=None, key=None, index_base=None, raw=None):
        """per caller position, under the definition or a fault, for this plan's key / index_base / rows or a control's"""
        if self.raw is not None:
            return [raw_weight(row, fault) for row in (self.raw if raw is None else raw)]
        key = self.key if key is None else key
        base = self.index_base if index_base is None else index_base
        return [weight(key, base + p, fault, index_base=base, gathered=self.gathered[p], shard_lo=self.shard_lo[p])
                for p in range(self.count)]

    def residues(self, fault=None, **control):
        """sum_p w_p x_p (mod r) of every group: the group passes its weighted check iff this is 0"""
        w = self.weights(fault, **control)
        return [sum(w[p] * self.coeffs[p] * self.defects[p] for p in g) % self.r for g in self.groups]

    def set_residues(self, fault=None):
        """the same sum over every set: 0 under the rule the plan was solved under"""
        w = self.weights(fault)
        return [sum(w[p] * self.coeffs[p] * self.defects[p] for p in s) % self.r for s in self.sets]

    def split(self, g):
        """group g holds part of a set and not all of it (the row across a group boundary): it must fail"""
        return any(0 < len(set(s) & set(g)) < len(s) for s in self.sets)

    def expect(self, fault=None, **control):
        """-> (verdict per caller position, groups failed, proofs re-verified) as the header defines them: a group that
        passes clears all its proofs, valid or not; the proofs of a group that fails get their exact verdicts"""
        verdicts, failed, redone = [0] * self.count, 0, 0
        for g, res in zip(self.groups, self.residues(fault, **control)):
            if res:
                failed, redone = failed + 1, redone + len(g)
                for p in g:
                    verdicts[p] = 1 if self.defects[p] else 0
        return verdicts, failed, redone

    def applicable(self):
        """the faults that change the weight of at least one defective proof of this plan"""
        if self.raw is not None:
            names = RAW_FAULTS
        else:
            names = FAULTS
        good = self.weights()
        return [f for f in names if any(a != b and d for a, b, d in zip(good, self.weights(f), self.defects))]

    def other_key(self):
        return hashlib.sha256(b"another key" + self.key).digest()


COUNTS = (2, 3, 255, 256, 257, 300)               # k_comb_fixed strides 256 threads over the proofs
BASES = (0, (1 << 32) - 2, (1 << 63) + 5)          # indices on both sides of 2^32 within one batch; the top bit of the index


def _rng(*what):
    return random.Random(" ".join(str(x) for x in what))


def _key(*what):
    return hashlib.sha256(("weight plan " + " ".join(str(x) for x in what)).encode()).digest()


def _kinds(ms, mix, members):
    """D everywhere; with mix, the first members of every set move a point instead: [A 1, V last, A 0, ..., last: A 2]"""
    kinds = [("D", 0)] * len(ms)
    if mix:
        for s in members:
            for i, p in enumerate(s[:3]):
                kinds[p] = (("A", 1), ("V", ms[p] - 1), ("A", 0))[i]
            if len(s) >= 4:
                kinds[s[-1]] = ("A", 2)
    return kinds


def combined_plans(curve, n, m):
    """bpp_verifier_run_combined, key form: one set = the whole batch"""
    out = []
    for count in COUNTS:
        for base in BASES:
            for mix in (False, True):
                name = "combined %s (%d,%d) count %d base %d %s" % (curve, n, m, count, base, "DAV" if mix else "D")
                ms, s = [m] * count, [list(range(count))]
                out.append(Plan(name, curve, n, ms, _kinds(ms, mix, s), s, _rng(name), key=_key(name), index_base=base))
    return out


def rank_plans(curve, n, m):
    """a cancelling batch split over two calls (ranks), each with index_base + its first proof"""
    out = []
    for count, lo, base in ((9, 4, 0), (6, 1, (1 << 32) - 3)):
        name = "ranks %s (%d,%d) count %d lo %d base %d" % (curve, n, m, count, lo, base)
        ms, s = [m] * count, [list(range(count))]
        out.append(Plan(name, curve, n, ms, _kinds(ms, True, s), s, _rng(name), key=_key(name), index_base=base,
                        cuts=[0, lo, count]))
    return out


GROUPED = ((2, 7), (4, 14), (32, 70))     # (group, count): the last group is short (of group 2: one proof, which stays valid)


def grouped_plans(curve, n, m, mix=True, challenges=None, tag="grouped"):
    """bpp_verifier_run_grouped: every group of two or more carries its own set; and one set across a group boundary.
    challenges: a function of the caller position (transcript proofs), None = literals"""
    out = []
    for i, (group, count) in enumerate(GROUPED):
        name = "%s %s (%d,%d) group %d count %d" % (tag, curve, n, m, group, count)
        ms = [m] * count
        sets = [list(range(lo, min(lo + group, count))) for lo in range(0, count, group) if min(lo + group, count) - lo >= 2]
        ch = [challenges(p) for p in range(count)] if challenges else None
        out.append(Plan(name, curve, n, ms, _kinds(ms, mix, sets), sets, _rng(name), key=_key(name), index_base=BASES[i],
                        group=group, challenges=ch))
    name = "%s %s (%d,%d) across a boundary" % (tag, curve, n, m)
    ms = [m] * 8
    ch = [challenges(p) for p in range(8)] if challenges else None
    out.append(Plan(name, curve, n, ms, [("D", 0)] * 8, [[3, 4]], _rng(name), key=_key(name), index_base=7, group=4,
                    challenges=ch))
    return out


MIXED_MS = (2, 1, 4, 1, 2, 4, 1, 2, 4)    # gathered: callers 1 3 6 | 0 4 7 | 2 5 8


def mixed_plans(curve, n, challenges=None, tag="mixed"):
    """bpp_verifier_run_grouped_mixed: classes interleaved in caller order, the groups (of the gathered order) hold proofs of
    different m and callers that are no neighbours; each group of two or more carries a set.  Kind D.  Per group size one
    plan solved under the definition and one under the `gathered` rule (which the definition must reject)."""
    out = []
    ms = list(MIXED_MS)
    order = gathered_order(ms, 0, len(ms))
    ch = [challenges(p) for p in range(len(ms))] if challenges else None
    for group, base in ((2, 5), (4, (1 << 32) - 4)):
        sets = [order[i:i + group] for i in range(0, len(order), group) if len(order[i:i + group]) >= 2]
        for rule in (None, "gathered"):
            name = "%s %s n %d group %d%s" % (tag, curve, n, group, " solved under " + rule if rule else "")
            out.append(Plan(name, curve, n, ms, [("D", 0)] * len(ms), sets, _rng(name), key=_key(name), index_base=base,
                            group=group, challenges=ch, solved_under=rule))
    return out


def pool_plans(curve, n, m, world, grouped, challenges=None):
    """the pool: sets in the second and the last shard, index_base non-zero; solved under the definition and under the
    `shard_local` rule (which the definition must reject).  grouped: containers, the shards cut by cost, groups of 4 inside
    each shard (kind D); else the combined check, the shards cut evenly, one set over members of both shards."""
    out = []
    count = 22 if grouped else 12
    ms = [m] * count
    cuts = cost_cuts(ms, world) if grouped else uniform_cuts(count, world)
    shards = sorted({1, world - 1})
    if grouped:     # the first group of the second and of the last shard, and the last shard's last (short) group
        sets = [list(range(cuts[s], cuts[s] + 4)) for s in shards]
        tail = cuts[world - 1] + (cuts[world] - cuts[world - 1]) // 4 * 4
        assert cuts[world] - tail >= 2 and tail > cuts[world - 1]
        sets.append(list(range(tail, cuts[world])))
    else:
        sets = [[p for s in shards for p in range(cuts[s] + 1, cuts[s + 1])]]
    ch = [challenges(p) for p in range(count)] if challenges else None
    for rule in (None, "shard_local"):
        name = "pool %s %s (%d,%d) world %d%s" % ("grouped" if grouped else "combined", curve, n, m, world,
                                                  " solved under " + rule if rule else "")
        kinds = [("D", 0)] * count if grouped else _kinds(ms, True, sets)
        out.append(Plan(name, curve, n, ms, kinds, sets, _rng(name), key=_key(name), index_base=(1 << 40) + 3,
                        group=4 if grouped else None, cuts=cuts, challenges=ch, solved_under=rule))
    return out


TOP_BITS = (1 << 127) | (1 << 63)


def raw_plans(curve, n, m):
    """caller-supplied weights: 128-bit values with the top bit of each half set, for the combined (group None) and the
    grouped entry; and a row of sixteen zero bytes, which weighs 1: a +d / -d pair under the rows [0, 1] cancels"""
    out = []
    for group, count in ((None, 5), (4, 10)):
        name = "raw %s (%d,%d) group %s" % (curve, n, m, group)
        rng = _rng(name)
        raw = [(rng.getrandbits(128) | TOP_BITS).to_bytes(16, "little") for _ in range(count)]
        ms = [m] * count
        sets = [list(range(count))] if group is None else [list(range(lo, min(lo + group, count))) for lo in range(0, count, group)]
        out.append(Plan(name, curve, n, ms, _kinds(ms, True, sets), sets, rng, raw=raw, group=group))
        name += " zero row"
        count = 2 if group is None else 6
        raw = [bytes(16), (1).to_bytes(16, "little")] + [(rng.getrandbits(128) | TOP_BITS).to_bytes(16, "little")] * (count - 2)
        plan = Plan(name, curve, n, [m] * count, [("D", 0)] * count, [[0, 1]], _rng(name), raw=raw, group=group)
        assert (plan.defects[0] + plan.defects[1]) % plan.r == 0           # +d / -d
        out.append(plan)
    return out


def plans(curve, n, m):
    """every plan of one uniform shape that needs literal challenges only (the transcript's and the mixed ones are built by
    their tests from the proofs' challenges): deterministic in its arguments"""
    return (combined_plans(curve, n, m) + rank_plans(curve, n, m) + grouped_plans(curve, n, m) + raw_plans(curve, n, m) +
            [p for world in (2, 3) for g in (False, True) for p in pool_plans(curve, n, m, world, g)])
