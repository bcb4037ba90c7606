"""-m gpu: WHICH weight the combined and the grouped check give WHICH proof (csrc/combined.hpp: comb_weight, k_comb_weights,
k_comb_weights_mixed, and the host code that passes index_base on), through the public entries alone.

Every other test of these paths compares verdicts with the exact per-proof path, which any consistent non-zero weights
satisfy.  Here every batch is a plan of tests/weight_cases.py: valid proofs, each given a defect that moves its MulVec along
h by a known multiple, the last defect of a set solved in big integers so that the set's weighted sum vanishes under the
DEFINITION of the weights.  Every proof of a set is invalid; the device accepts the set iff it used exactly those weights
for exactly those proofs.  tests/test_weight_cases_cpu.py shows, without a GPU, that each plan cancels under the definition
and under none of the wrong rules of weight_cases.FAULTS that applies to it.  Every expected word below is plan.expect(): big
integers, nothing learned from a run; the controls (the next index_base, another key, a set solved under a wrong rule) are
the same buffers or the same construction with the outcome reversed."""

import functools

import numpy as np
import pytest

import oracle as O
import pyref as P
import verdict_corpus as VC
import weight_cases as WC
from gpu_util import need_gpu, run_combined_device, run_grouped_device, run_verifier_device

pytestmark = pytest.mark.gpu

CURVES = ("bls12_381", "secp256k1", "ed25519")
N, CAP, WB, DISTINCT = 8, 4, 5, 3


# ---- valid proofs and the shifts along h ----------------------------------------------------------------------------------
class Material:
    """DISTINCT valid proofs of shape (N, m) under the reference key: the C oracle's, the device prover's on edwards25519
    (which the C oracle does not have).  recs (DISTINCT, 3 + 2k + m, PW), scs (DISTINCT, 3, 4); challenges: per proof what the
    transcript derives (pyref), None under the literals"""

    def __init__(self, cname, m, transcript):
        self.cname, self.m, self.cid = cname, m, O.CURVE_IDS[cname]
        self.cp = cp = VC.Corpus(cname, N, m, transcript)
        self.k = cp.k
        vals = [[(41 * t + 13 * j + m) % (1 << N) for j in range(m)] for t in range(DISTINCT)]
        gams = [[3 + 5 * t + j for j in range(m)] for t in range(DISTINCT)]
        if cname == "ed25519":
            import bulletproofsplus_amd as B
            a = B.Arith(cname)
            bv = B.BatchVerifier(B.PublicKey.from_points(a, cp.gh, cp.G, cp.H), N, m, window_bits=WB)
            pts, self.scs, V = bv.prove_batch(vals, gams, transcript=transcript)
            bv.close()
            self.recs = np.concatenate([pts, V], axis=1)
        else:
            O.set_transcript(transcript)
            try:
                out = [O.range_prove(cp.opk, N, v, g) for v, g in zip(vals, gams)]
                assert all(O.range_verify(cp.opk, N, m, pts, sc, V) == 0 for pts, sc, V in out)
            finally:
                O.set_transcript(False)
            self.recs = np.stack([np.concatenate([pts, V]) for pts, _, V in out])
            self.scs = np.stack([np.array(sc, copy=True) for _, sc, _ in out])
        self.challenges = [None] * DISTINCT
        if transcript:
            ppk = cp.ppk if cname == "ed25519" else P.PublicKey(cp.grp, N * m)
            nrec = 3 + 2 * self.k
            self.challenges = [WC.fs_challenges(cname, N, m, ppk, O.wire_to_points(self.cid, rec[:nrec]),
                                                O.wire_to_points(self.cid, rec[nrec:])) for rec in self.recs]

    def shifted(self, w, t):
        """the wire point w + t h"""
        h = self.cp.gh[1]
        if self.cname != "ed25519":
            return O.point_add(self.cid, w, O.point_mul(self.cid, h, t))
        g = self.cp.grp
        return O.point_to_wire(2, g.add(O.wire_to_point(2, w), g.mul(O.wire_to_point(2, h), t)))


@functools.lru_cache(maxsize=None)
def _material(cname, m, transcript=False):
    return Material(cname, m, transcript)


def _apply(plan, mats):
    """the plan's batch -> (records per caller position, scalars (count, 3, 4)): base proof pick[p] of its class with the
    plan's defect of position p"""
    pick = WC.pick(plan.ms, DISTINCT)
    recs, scs = [], []
    for p, m in enumerate(plan.ms):
        mat = mats[m]
        rec, sc = mat.recs[pick[p]].copy(), mat.scs[pick[p]].copy()
        (kind, j), d = plan.kinds[p], plan.defects[p]
        if d and kind == "D":
            dp = O.wire_to_scalars(sc[2])[0]
            assert dp < plan.r
            sc[2] = O.scalars_to_wire([(dp + d) % plan.r])[0]         # canonical
        elif d:
            at = j if kind == "A" else 3 + 2 * mat.k + j
            rec[at] = mat.shifted(rec[at], d)
        recs.append(rec)
        scs.append(sc)
    return recs, np.stack(scs)


def _chal(mats, ms):
    """the plan builders' `challenges` argument for transcript proofs replicated by WC.pick"""
    pick = WC.pick(ms, DISTINCT)
    return lambda p: mats[ms[p]].challenges[pick[p]]


def _engine(B, cname, m):
    cp = _material(cname, m).cp
    a = B.Arith(cname)
    return a, B.BatchVerifier(B.PublicKey.from_points(a, cp.gh, cp.G, cp.H), N, m, window_bits=WB)


def _all_invalid(torch, bv, plan, recs, scs):
    """the exact path on a uniform plan's batch: precisely the defective proofs fail -- every member of a set is invalid"""
    exact, _, _ = run_verifier_device(torch, bv, np.stack(recs), scs, want_scalars=False, want_result=False)
    assert exact.tolist() == [1 if d else 0 for d in plan.defects], plan.name


def _flag(bv, part):
    return int(part.view(np.uint32)[bv.partial_bytes() // 4 - 4])


# ---- bpp_verifier_run_combined, key form -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,m", [(c, m) for c in CURVES for m in (1, 2)])
def test_combined_key_form(cname, m):
    """counts 2, 3, 255, 256, 257, 300 x index_base 0, 2^32 - 2, 2^63 + 5 x kinds D / D with A and V: d_ok 0 and a clear validity
    word; the same buffers under index_base + 1 and under another key: d_ok 1"""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    a, bv = _engine(B, cname, m)
    mats = {m: _material(cname, m)}
    plans = WC.combined_plans(cname, N, m)
    assert len(plans) == 36
    for i, plan in enumerate(plans):
        recs, scs = _apply(plan, mats)
        recs = np.stack(recs)
        if i % 12 == 7:
            _all_invalid(torch, bv, plan, recs, scs)
        assert plan.expect()[1] == 0 and plan.expect(index_base=plan.index_base + 1)[1] == 1
        assert plan.expect(key=plan.other_key())[1] == 1
        ok, part = run_combined_device(torch, bv, recs, scs, key=plan.key, index_base=plan.index_base)
        assert (ok, _flag(bv, part)) == (0, 0), plan.name
        ok, part = run_combined_device(torch, bv, recs, scs, key=plan.key, index_base=plan.index_base + 1)
        assert (ok, _flag(bv, part)) == (1, 0), plan.name
        ok, _ = run_combined_device(torch, bv, recs, scs, key=plan.other_key(), index_base=plan.index_base)
        assert ok == 1, plan.name
    bv.close()


@pytest.mark.parametrize("cname,m", [("bls12_381", 2), ("secp256k1", 1), ("ed25519", 2)])
def test_combined_two_ranks(cname, m):
    """a cancelling batch split over two calls: index_base + lo for the second gives partials that sum to the identity, the
    same index_base for both does not"""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    a, bv = _engine(B, cname, m)
    dev = torch.device("cuda:0")
    d_ok = torch.full((1,), 7, dtype=torch.int32, device=dev)
    for plan in WC.rank_plans(cname, N, m):
        recs, scs = _apply(plan, {m: _material(cname, m)})
        recs = np.stack(recs)
        lo = plan.cuts[1]
        assert plan.expect()[1] == 0 and plan.expect("shard_local")[1] == 1
        for second, want in ((plan.index_base + lo, 0), (plan.index_base, 1)):
            ok0, p0 = run_combined_device(torch, bv, recs[:lo], scs[:lo], key=plan.key, index_base=plan.index_base)
            ok1, p1 = run_combined_device(torch, bv, recs[lo:], scs[lo:], key=plan.key, index_base=second)
            assert (ok0, ok1) == (1, 1)                                 # neither share cancels alone
            d_parts = torch.from_numpy(np.concatenate([p0, p1])).to(dev)
            bv.sum_partials_device(d_parts.data_ptr(), 2, d_ok.data_ptr())
            torch.cuda.synchronize()
            assert int(d_ok.item()) == want, (plan.name, second)
    bv.close()


# ---- bpp_verifier_run_grouped, _begin / _finish ----------------------------------------------------------------------------
@pytest.mark.parametrize("cname,m", [(c, m) for c in CURVES for m in (1, 2)])
def test_grouped_key_form(cname, m):
    """groups of 2, 4, 32 with a short last group, a set per group: verdicts all 0 and stats (0, 0) although every member is
    invalid; under index_base + 1 every such group fails and is redone.  And a set across a group boundary: both groups fail."""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    a, bv = _engine(B, cname, m)
    for plan in WC.grouped_plans(cname, N, m):
        recs, scs = _apply(plan, {m: _material(cname, m)})
        recs = np.stack(recs)
        _all_invalid(torch, bv, plan, recs, scs)
        want = plan.expect()
        if plan.sets != [[3, 4]]:
            assert want == ([0] * plan.count, 0, 0)
        control = plan.expect(index_base=plan.index_base + 1)
        sized = [g for g in plan.groups if len(g) >= 2] if plan.sets != [[3, 4]] else plan.groups
        assert control == ([1 if d else 0 for d in plan.defects], len(sized), sum(len(g) for g in sized))
        for halves in (False, True):
            ok, failed, redone = run_grouped_device(torch, bv, recs, scs, plan.group, key=plan.key, index_base=plan.index_base,
                                                    halves=halves)
            assert (ok.tolist(), failed, redone) == want, (plan.name, halves)
            ok, failed, redone = run_grouped_device(torch, bv, recs, scs, plan.group, key=plan.key,
                                                    index_base=plan.index_base + 1, halves=halves)
            assert (ok.tolist(), failed, redone) == control, (plan.name, halves)
        ok, failed, redone = run_grouped_device(torch, bv, recs, scs, plan.group, key=plan.other_key(), index_base=plan.index_base)
        assert (ok.tolist(), failed, redone) == plan.expect(key=plan.other_key()) == control, plan.name
    bv.close()


# ---- caller-supplied weights ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,m", [("bls12_381", 1), ("secp256k1", 2), ("ed25519", 1)])
def test_caller_supplied_weights(cname, m):
    """128-bit rows with the top bit of each half set, and a row of sixteen zero bytes that weighs 1, through the combined and
    the grouped entry; with bit 64 of the first row flipped the first set no longer cancels"""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    a, bv = _engine(B, cname, m)
    for plan in WC.raw_plans(cname, N, m):
        recs, scs = _apply(plan, {m: _material(cname, m)})
        recs = np.stack(recs)
        _all_invalid(torch, bv, plan, recs, scs)
        rows = np.frombuffer(b"".join(plan.raw), dtype=np.uint64).reshape(plan.count, 2).copy()
        want = plan.expect()
        assert want == ([0] * plan.count, 0, 0)
        other = [(int.from_bytes(plan.raw[0], "little") ^ (1 << 64)).to_bytes(16, "little")] + plan.raw[1:]
        control = plan.expect(raw=other)
        assert control[1] == 1
        moved = rows.copy()
        moved[0, 1] ^= np.uint64(1)
        for w, exp in ((rows, want), (moved, control)):
            if plan.group is None:
                ok, part = run_combined_device(torch, bv, recs, scs, weights=w)
                assert (ok, _flag(bv, part)) == (1 if exp[1] else 0, 0), plan.name
            else:
                ok, failed, redone = run_grouped_device(torch, bv, recs, scs, plan.group, weights=w)
                assert (ok.tolist(), failed, redone) == exp, plan.name
    bv.close()


# ---- bpp_verifier_run_grouped_mixed -----------------------------------------------------------------------------------------
def _cap_engine(B, cname):
    return _engine(B, cname, CAP)


def _upload(torch, a, recs, scs):
    dev = torch.device("cuda:0")
    pts = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.uint64).reshape(-1, a.PW) for r in recs]))
    return (torch.from_numpy(pts.view(np.int64)).to(dev),
            torch.from_numpy(np.ascontiguousarray(scs, dtype=np.uint64).view(np.int64)).to(dev))


@pytest.mark.parametrize("cname", CURVES)
def test_grouped_mixed_key_form(cname):
    """classes interleaved in caller order, sets of proofs of different m that are neighbours in gathered order only: the PRF
    index is index_base + the CALLER's position.  The same construction solved for the gathered position must fail."""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    a, bv = _cap_engine(B, cname)
    mats = {m: _material(cname, m) for m in (1, 2, 4)}
    dev = torch.device("cuda:0")
    for plan in WC.mixed_plans(cname, N):
        assert B.mixed_groups(plan.ms, plan.group).tolist() == [plan.gathered[p] // plan.group for p in range(plan.count)]
        recs, scs = _apply(plan, mats)
        d_pts, d_sc = _upload(torch, a, recs, scs)
        wsb = bv.grouped_mixed_workspace_bytes(plan.ms, plan.group)
        assert wsb > 0
        d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        sized = [g for g in plan.groups if len(g) >= 2]
        rejected = ([1 if d else 0 for d in plan.defects], len(sized), sum(len(g) for g in sized))
        runs = [(plan.key, plan.index_base, plan.expect())]
        if plan.solved_under is None:
            assert plan.expect() == ([0] * plan.count, 0, 0)
            runs += [(plan.key, plan.index_base + 1, rejected), (plan.other_key(), plan.index_base, rejected)]
            assert plan.expect(index_base=plan.index_base + 1) == plan.expect(key=plan.other_key()) == rejected
        else:
            assert plan.expect() == rejected and plan.expect("gathered") == ([0] * plan.count, 0, 0)
        for key, base, want in runs:
            d_ok = torch.full((plan.count,), 7, dtype=torch.int32, device=dev)
            failed, redone = bv.run_grouped_mixed_device(d_pts.data_ptr(), d_sc.data_ptr(), plan.ms, key, base, d_ok.data_ptr(),
                                                         d_ws.data_ptr(), wsb, group=plan.group,
                                                         stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert (d_ok.cpu().tolist(), failed, redone) == want, (plan.name, base)
    bv.close()


# ---- behind the decoder: kind D written into the container bytes -----------------------------------------------------------
def _containers(B, a, plan, mats):
    """the plan's batch as containers and compressed commitments, per caller position: the valid proof encoded, then delta'
    (its last 32 bytes) replaced by delta' + d"""
    pick = WC.pick(plan.ms, DISTINCT)
    blobs, comms = [], []
    for p, m in enumerate(plan.ms):
        mat = mats[m]
        nrec = 3 + 2 * mat.k
        rec, sc = mat.recs[pick[p]], mat.scs[pick[p]]
        blob = B.encode_proofs(a, N, m, rec[:nrec], sc)[0].tobytes()
        dp = int.from_bytes(blob[-32:], "little")
        assert plan.kinds[p] == ("D", 0) and dp == O.wire_to_scalars(sc[2])[0]
        blobs.append(blob[:-32] + ((dp + plan.defects[p]) % plan.r).to_bytes(32, "little"))
        comms.append(B.compress_points(a, rec[nrec:]).tobytes())
    return blobs, comms


def _u8(chunks):
    return np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()


@pytest.mark.parametrize("transcript", (False, True))
@pytest.mark.parametrize("cname", CURVES)
def test_serialized_grouped_key_form(cname, transcript):
    """bpp_range_verify_batch_serialized_grouped_device, shape (8, 2): under the transcript c_h = -e^-2 with the proof's own e"""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    m = 2
    a, bv = _engine(B, cname, m)
    mats = {m: _material(cname, m, transcript)}
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for plan in WC.grouped_plans(cname, N, m, mix=False, challenges=_chal(mats, [m] * 70) if transcript else None,
                                 tag="serialized"):
        blobs, comms = _containers(B, a, plan, mats)
        d_bl, d_cm = torch.from_numpy(_u8(blobs)).to(dev), torch.from_numpy(_u8(comms)).to(dev)
        exact = bv.verify_serialized(_u8(blobs), _u8(comms), transcript=transcript)
        assert exact.tolist() == [1 if d else 0 for d in plan.defects], plan.name
        wsb = bv.serialized_grouped_workspace_bytes(plan.count, plan.group)
        d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        control = plan.expect(index_base=plan.index_base + 1)
        assert control[0] == exact.tolist() and control[1] >= 2
        for base, want in ((plan.index_base, plan.expect()), (plan.index_base + 1, control)):
            d_ok = torch.full((plan.count,), 7, dtype=torch.int32, device=dev)
            stats = bv.verify_serialized_grouped_device(d_bl.data_ptr(), d_cm.data_ptr(), plan.count, d_ok.data_ptr(),
                                                        d_ws.data_ptr(), wsb, plan.key, base, plan.group, stream,
                                                        transcript=transcript)
            torch.cuda.synchronize()
            assert (d_ok.cpu().tolist(),) + tuple(stats) == want, (plan.name, base)
    bv.close()


@pytest.mark.parametrize("transcript", (False, True))
@pytest.mark.parametrize("cname", CURVES)
def test_serialized_grouped_mixed_key_form(cname, transcript):
    """bpp_range_verify_batch_serialized_grouped_mixed_device on the interleaved classes: caller positions, not gathered ones"""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    a, bv = _cap_engine(B, cname)
    mats = {m: _material(cname, m, transcript) for m in (1, 2, 4)}
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    ms = list(WC.MIXED_MS)
    for plan in WC.mixed_plans(cname, N, challenges=_chal(mats, ms) if transcript else None, tag="serialized mixed"):
        blobs, comms = _containers(B, a, plan, mats)
        d_bl, d_cm = torch.from_numpy(_u8(blobs)).to(dev), torch.from_numpy(_u8(comms)).to(dev)
        wsb = bv.serialized_grouped_mixed_workspace_bytes(plan.ms, plan.group)
        assert wsb > 0
        d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        sized = [g for g in plan.groups if len(g) >= 2]
        rejected = ([1 if d else 0 for d in plan.defects], len(sized), sum(len(g) for g in sized))
        if plan.solved_under is None:
            runs = [(plan.index_base, plan.expect()), (plan.index_base + 1, plan.expect(index_base=plan.index_base + 1))]
            assert runs[0][1] == ([0] * plan.count, 0, 0) and runs[1][1] == rejected
        else:
            runs = [(plan.index_base, plan.expect())]
            assert runs[0][1] == rejected
        for base, want in runs:
            d_ok = torch.full((plan.count,), 7, dtype=torch.int32, device=dev)
            stats = bv.verify_serialized_grouped_mixed_device(d_bl.data_ptr(), d_cm.data_ptr(), plan.ms, d_ok.data_ptr(),
                                                              d_ws.data_ptr(), wsb, plan.key, base, plan.group, stream,
                                                              transcript=transcript)
            torch.cuda.synchronize()
            assert (d_ok.cpu().tolist(),) + tuple(stats) == want, (plan.name, base)
    bv.close()


# ---- the pool ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", (2, 3))
@pytest.mark.parametrize("cname", CURVES)
def test_pool_weights_are_the_callers(cname, world):
    """VerifierPool(devices=(0,) * world), the grouped bytes mode and the combined mode, sets in the second and the last shard,
    index_base non-zero: proof i is weighted by index_base + i whatever the cut.  The same construction solved for an index
    that forgets the shard's first proof must fail."""
    need_gpu()
    import bulletproofsplus_amd as B
    m = 2
    mat = _material(cname, m)
    a = B.Arith(cname)
    pool = B.VerifierPool(B.PublicKey.from_points(a, mat.cp.gh, mat.cp.G, mat.cp.H), N, m, window_bits=WB, devices=(0,) * world)
    for plan in WC.pool_plans(cname, N, m, world, grouped=True):
        assert pool.cuts(plan.ms).tolist() == plan.cuts
        blobs, comms = _containers(B, a, plan, {m: mat})
        want = plan.expect()
        rejected = [1 if d else 0 for d in plan.defects]
        if plan.solved_under:
            assert want == (rejected, len(plan.sets), sum(len(s) for s in plan.sets)) and len(plan.sets) == world
        else:
            assert want == ([0] * plan.count, 0, 0)
        ok, stats = pool.verify_serialized_mixed(_u8(blobs), _u8(comms), plan.ms, grouped=True, weight_key=plan.key,
                                                 index_base=plan.index_base, group=plan.group, return_stats=True)
        assert (ok.tolist(),) + tuple(stats) == want, plan.name
        if plan.solved_under is None:
            ok = pool.verify_serialized_mixed(_u8(blobs), _u8(comms), plan.ms, grouped=True, weight_key=plan.key,
                                              index_base=plan.index_base + 1, group=plan.group)
            assert ok.tolist() == plan.expect(index_base=plan.index_base + 1)[0] == rejected, plan.name
    for plan in WC.pool_plans(cname, N, m, world, grouped=False):
        assert pool.cuts(None, plan.count).tolist() == plan.cuts
        recs, scs = _apply(plan, {m: mat})
        want = plan.expect()[1]
        assert want == (1 if plan.solved_under else 0)
        assert pool.verify_combined(np.stack(recs), scs, weight_key=plan.key, index_base=plan.index_base) == want, plan.name
        if plan.solved_under is None:
            assert plan.expect(index_base=plan.index_base + 1)[1] == 1
            assert pool.verify_combined(np.stack(recs), scs, weight_key=plan.key, index_base=plan.index_base + 1) == 1, plan.name
    pool.close()
