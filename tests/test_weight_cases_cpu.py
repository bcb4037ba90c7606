"""The weight plans (tests/weight_cases.py) in big integers, no GPU: every plan's sets cancel under the definition of the
weights and under no wrong rule that applies to the plan -- the evidence that the batches test_gpu_weights.py hands to the
device tell the definition from each of those rules -- and the plans have the structure they exist for."""

import hashlib

import numpy as np
import pytest

import oracle as O
import pyref as P
import scalar_cases as SC
import weight_cases as WC
from test_gpu_weights import _apply, _material

N = 8
SHAPES = [(c, m) for c in SC.CURVES for m in (1, 2)]
DIGEST_FAULTS = ["one", "low64", "low32", "bytes16_32", "big_endian", "no_tag", "no_key"]


def _defective(plan, g):
    return any(plan.defects[p] for p in g)


def _check(plan):
    """cancellation under the rule the plan was solved under; under every other rule that applies, none"""
    r = plan.r
    assert all(0 <= d < r for d in plan.defects) and all(plan.defects[p] for s in plan.sets for p in s)
    assert sum(1 for d in plan.defects if d) == sum(len(s) for s in plan.sets)
    if plan.solved_under is not None:
        # a control: it cancels under the wrong rule, group by group, and the definition rejects every group that carries it
        assert not any(plan.residues(plan.solved_under)) and not any(plan.set_residues(plan.solved_under)), plan.name
        assert all(bool(res) == _defective(plan, g) for g, res in zip(plan.groups, plan.residues())), plan.name
        return []
    assert not any(plan.set_residues()), plan.name
    # a group passes unless a set is split over its boundary
    assert all(bool(res) == plan.split(g) for g, res in zip(plan.groups, plan.residues())), plan.name
    good = plan.weights()
    applied = plan.applicable()
    for f in applied:
        bad = plan.weights(f)
        for g, res in zip(plan.groups, plan.residues(f)):
            if any(plan.defects[p] and good[p] != bad[p] for p in g) and not plan.split(g):
                assert res, (plan.name, f, g)           # a plan that fails to separate a fault that applies is a bug in the plan
    if plan.key is not None:       # the controls of the key form: the next index_base, another key
        for kw in (dict(index_base=plan.index_base + 1), dict(key=plan.other_key())):
            assert all(bool(res) == _defective(plan, g) for g, res in zip(plan.groups, plan.residues(**kw))), (plan.name, kw)
    return applied


def test_the_definition_and_its_faults_differ():
    key = hashlib.sha256(b"k").digest()
    dg = hashlib.sha256(key + b"bppw" + (5).to_bytes(8, "little")).digest()
    assert WC.weight(key, 5) == int.from_bytes(dg[:16], "little")
    base, idx = (1 << 32) + 9, (1 << 32) + 12
    seen = {None: WC.weight(key, idx, index_base=base, gathered=1, shard_lo=5)}
    for f in WC.FAULTS:
        seen[f] = WC.weight(key, idx, f, index_base=base, gathered=1, shard_lo=5)
    assert len(set(seen.values())) == len(seen)                 # each rule is a different weight
    assert seen["low64"] == seen[None] & WC.M64 and seen["low32"] == seen[None] & 0xFFFFFFFF
    assert seen["index32"] == WC.weight(key, 12) and seen["no_base"] == WC.weight(key, 3)
    assert seen["gathered"] == WC.weight(key, base + 1) and seen["shard_local"] == WC.weight(key, idx - 5)
    assert WC.raw_weight(bytes(16)) == 1 and WC.raw_weight(bytes(16), "zero_stays_zero") == 0
    assert WC.raw_weight(b"\x01" + bytes(14) + b"\x80") == (1 << 127) + 1


@pytest.mark.parametrize("curve,m", SHAPES)
def test_coefficients_from_the_restatement(curve, m):
    """c_h by differencing is -1 (m = 1) or -e^-2 (m > 1); the point kinds read the MulVec scalar of their point; pyref's
    verify_mulvec over the shadow group gives the same numbers"""
    r = SC.order(curve)
    rng = WC._rng("coefficients", curve, m)
    for ch in (None, (rng.randrange(1, r), rng.randrange(1, r), rng.randrange(1, r), [rng.randrange(1, r) for _ in range(SC.log2(N * m))])):
        y, z, e, er = ch if ch else WC.literal_challenges(N, m)
        want = r - 1 if m == 1 else -pow(e, -2, r) % r
        assert WC.coefficient(curve, N, m, "D", 0, ch) == want
        mv = SC.range_scalars(curve, N, m, y, z, e, er, [0, 0, 0])
        head = [mv[2], mv[1], mv[0]] if m == 1 else mv[:3]
        assert [WC.coefficient(curve, N, m, "A", j, ch) for j in range(3)] == head
        assert [WC.coefficient(curve, N, m, "V", j, ch) for j in range(m)] == mv[len(mv) - m:]


@pytest.mark.parametrize("curve", ("bls12_381", "secp256k1"))
def test_every_defect_moves_the_mulvec_along_h_by_its_coefficient(curve):
    """the instrument itself, on the full curve with the C oracle: a proof with a defect of any kind is rejected, and its
    MulVec is (coefficient * defect) h -- through the very code that builds the device's batches"""
    cid = O.CURVE_IDS[curve]
    for m in (1, 2, 4):
        mat = _material(curve, m)
        kinds = [("D", 0), ("A", 0), ("A", 1), ("A", 2)] + [("V", j) for j in range(m)]
        plan = WC.Plan("probe", curve, N, [m] * len(kinds), kinds, [list(range(len(kinds)))], WC._rng("probe", curve, m),
                       key=bytes(32))
        recs, scs = _apply(plan, {m: mat})
        nrec = 3 + 2 * mat.k
        for p, (rec, sc) in enumerate(zip(recs, scs)):
            rc, _, res = O.range_verify(mat.cp.opk, N, m, rec[:nrec], sc, rec[nrec:], want_result=True)
            x = plan.coeffs[p] * plan.defects[p] % plan.r
            assert rc == 1 and x and np.array_equal(res, O.point_mul(cid, mat.cp.gh[1], x)), (m, kinds[p])


@pytest.mark.parametrize("curve,m", SHAPES)
def test_uniform_plans_cancel_under_the_definition_only(curve, m):
    plans = WC.plans(curve, N, m)
    again = WC.plans(curve, N, m)
    assert [p.defects for p in plans] == [p.defects for p in again]        # deterministic in the arguments
    applied = {p.name: _check(p) for p in plans}
    comb = [p for p in plans if p.name.startswith("combined")]
    assert sorted({p.count for p in comb}) == [2, 3, 255, 256, 257, 300]   # both sides of 256
    for p in comb:
        assert set(DIGEST_FAULTS) <= set(applied[p.name]), p.name
        assert ("no_base" in applied[p.name]) == (p.index_base != 0)
        lo, hi = p.index_base, p.index_base + p.count - 1
        if lo < 1 << 32 <= hi:                                             # indices on both sides of 2^32 within one batch
            assert "index32" in applied[p.name]
    assert any(p.index_base < 1 << 32 <= p.index_base + p.count - 1 for p in comb)
    assert any(p.index_base >> 63 and "index32" in applied[p.name] for p in comb)
    # a weight with the top bit of each 64-bit half set, in the key form and in every raw row
    assert any(w >> 127 and (w >> 63) & 1 for p in comb for w in p.weights())
    raw = [p for p in plans if p.name.startswith("raw")]
    assert len(raw) == 4 and {p.group for p in raw} == {None, 4}
    for p in raw:
        if "zero row" in p.name:
            assert p.weights()[:2] == [1, 1] and applied[p.name] == ["zero_stays_zero"]
        else:
            assert all(w >> 127 and (w >> 63) & 1 for w in p.weights())
    # the point kinds and the delta' kind share every combined "DAV" set, every rank set and every larger group
    for p in plans:
        if " DAV" in p.name or p.name.startswith("ranks"):
            assert {"D", "A", "V"} <= {kd for kd, _ in p.kinds} or p.count < 4
            assert len({kd for kd, _ in p.kinds}) >= 2
    grouped = [p for p in plans if p.name.startswith("grouped")]
    assert [p.group for p in grouped] == [2, 4, 32, 4]
    for p in grouped[:3]:
        assert p.count % p.group and len(p.groups[-1]) < p.group          # the last group is short
        assert [s for s in p.sets] == [g for g in p.groups if len(g) >= 2]
    across = grouped[3]
    assert across.sets == [[3, 4]] and across.expect() == ([0, 0, 0, 1, 1, 0, 0, 0], 2, 8)   # both groups fail
    for p in plans:
        if p.name.startswith("ranks") or p.name.startswith("pool"):
            if p.solved_under is None:
                assert "shard_local" in applied[p.name] and ("no_base" in applied[p.name] or p.index_base == 0)
            assert all(p.shard_lo[q] > 0 for s in p.sets for q in s[-1:])  # the sets reach the second or the last shard
    pool = [p for p in plans if p.name.startswith("pool")]
    assert len(pool) == 8 and all(p.index_base for p in pool)
    for p in pool:
        world = len(p.cuts) - 1
        shards = {max(s for s in range(world) if p.cuts[s] <= q) for st in p.sets for q in st}
        assert shards == {1, world - 1}, p.name


@pytest.mark.parametrize("curve", SC.CURVES)
def test_mixed_plans_cancel_under_the_definition_only(curve):
    plans = WC.mixed_plans(curve, N)
    assert [p.solved_under for p in plans] == [None, "gathered", None, "gathered"]
    r = SC.order(curve)
    for p in plans:
        applied = _check(p)
        if p.solved_under is None:
            assert "gathered" in applied and set(DIGEST_FAULTS) <= set(applied)
        # classes interleaved in caller order; sets of proofs of different m (coefficients -1 and -e^-2); members that are
        # neighbours in gathered order but not in caller order
        assert p.ms != sorted(p.ms) and sorted(set(p.ms)) == [1, 2, 4]
        assert any(len({p.ms[q] for q in s}) > 1 for s in p.sets)
        assert any({p.coeffs[q] for q in s} >= {r - 1, -pow(P.Transcript.E_FINAL, -2, r) % r} for s in p.sets)
        assert any(abs(a - b) > 1 and abs(p.gathered[a] - p.gathered[b]) == 1 for s in p.sets for a, b in zip(s, s[1:]))
    assert any(p.index_base < 1 << 32 <= p.index_base + p.count - 1 for p in plans)


# ---- under the transcript: delta' is drawn after the last challenge ------------------------------------------------------
def _transcript_proofs(curve, m, distinct):
    """`distinct` proofs of the C oracle under the transcript -> [(points (3 + 2k) affine, V affine, scalars [r', s', d'])]"""
    cid = O.CURVE_IDS[curve]
    opk = O.PublicKey(cid, N * m)
    out = []
    O.set_transcript(True)
    try:
        for t in range(distinct):
            pts, sc, V = O.range_prove(opk, N, [(29 * t + 7 * j + m) % 256 for j in range(m)], [3 + t + j for j in range(m)])
            assert O.range_verify(opk, N, m, pts, sc, V) == 0
            out.append((O.wire_to_points(cid, pts), O.wire_to_points(cid, V), O.wire_to_scalars(sc)))
    finally:
        O.set_transcript(False)
    return out


@pytest.mark.parametrize("curve", ("bls12_381", "secp256k1"))
def test_transcript_plans_and_the_shifted_container(curve):
    G = P.make_group(curve, False)
    r = SC.order(curve)
    chal = {}
    for m in (1, 2, 4):
        ppk = P.PublicKey(G, N * m)
        proofs = _transcript_proofs(curve, m, 3)
        chal[m] = [WC.fs_challenges(curve, N, m, ppk, pts, V) for pts, V, _ in proofs]
        assert len({c[2] for c in chal[m]}) == 3                   # a final challenge of its own per proof
        # the container with delta' moved decodes to the same points, hence to the same challenges, and to delta' + d
        pts, V, (rp, sp, dp) = proofs[0]
        k = SC.log2(N * m)
        proof = P.RangeProof(pts[0], P.WeightedInnerProductProof(pts[3:3 + k], pts[3 + k:], pts[1], pts[2], rp, sp, dp))
        blob = P.encode_proof(P.CURVES[curve], N, m, proof)
        assert int.from_bytes(blob[-32:], "little") == dp
        d = WC._rng("shift", curve, m).randrange(1, r)
        moved = blob[:-32] + ((dp + d) % r).to_bytes(32, "little")
        back = P.decode_proof(P.CURVES[curve], G, N, m, moved)
        assert back is not None and back.proof.d_prime == (dp + d) % r and (back.proof.r_prime, back.proof.s_prime) == (rp, sp)
        w = back.proof
        assert WC.fs_challenges(curve, N, m, ppk, [back.A, w.A, w.B] + list(w.L_vec) + list(w.R_vec), V) == chal[m][0]
    for m in (1, 2):
        plans = WC.grouped_plans(curve, N, m, mix=False, challenges=lambda p: chal[m][p % 3], tag="serialized")
        for p in plans:
            _check(p)
            assert {kd for kd, _ in p.kinds} == {"D"}
            if m > 1:
                assert len({p.coeffs[q] for q in range(p.count)}) == 3     # -e^-2 with the proof's own e
    ms = list(WC.MIXED_MS)
    seen = {m: 0 for m in (1, 2, 4)}
    per = []
    for m in ms:
        per.append(chal[m][seen[m] % 3])
        seen[m] += 1
    for p in WC.mixed_plans(curve, N, challenges=lambda q: per[q], tag="serialized mixed"):
        _check(p)
