"""-m gpu: the grouped check over mixed batches (bpp_verifier_run_grouped_mixed, and behind the decoder
bpp_range_verify_batch_serialized_grouped_mixed_device): proof i of shape (n, m_i) against one (n, m) verifier's tables, one
weighted check per group of neighbours of the batch gathered by aggregation size, an exact pass over the groups that fail.

The bar throughout is the verdict vector of the exact mixed call (run_mixed_device, itself pinned to the definition by
tests/test_gpu_mixed.py; verify_serialized_mixed_device for bytes) on the same buffers with the same subgroup-check
setting, AND the exact `stats`: the verdicts alone cannot see a first pass that wrongly fails valid groups, because the
second pass repairs it -- a wrong generator mapping in the row kernel shows up only as failed != expected.  So every case
asserts failed == the number of groups (by mixed_groups) holding at least one proof the exact call rejects, and redone ==
the sizes of those groups."""

import functools
import hashlib

import numpy as np
import pytest

import oracle as O
import verdict_corpus as VC
from gpu_util import need_gpu, run_grouped_device
from test_gpu_mixed import _interleave, _record, _run_mixed
from test_gpu_serialized_mixed import _run as _run_serialized_mixed, _u8

pytestmark = pytest.mark.gpu

CURVES = ("bls12_381", "secp256k1", "ed25519")
N, CAP, WB = 8, 4, 5
CLASSES = (1, 2, 4)


@functools.lru_cache(maxsize=None)
def _corpora(cname, transcript=False):
    return {m: VC.corpus(cname, N, m, transcript=transcript) for m in CLASSES}


def _key(seed):
    return hashlib.sha256(b"grouped mixed %d" % seed).digest()


def _predict(ms, group, exact):
    """-> (failed, redone) from the documented partition and the exact call's vector"""
    from bulletproofsplus_amd import mixed_groups
    g = mixed_groups(ms, group)
    hit = sorted(set(g[np.asarray(exact) != 0].tolist()))
    return len(hit), int(sum(int((g == h).sum()) for h in hit))


def _upload(torch, bv, recs, scs, challenges=None):
    dev = torch.device("cuda:0")
    PW = bv.arith.PW
    pts = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.uint64).reshape(-1, PW) for r in recs]))
    d_pts = torch.from_numpy(pts.view(np.int64)).to(dev)
    d_sc = torch.from_numpy(np.ascontiguousarray(scs, dtype=np.uint64).view(np.int64)).to(dev)
    d_ch = None
    if challenges is not None:
        flat = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint64).reshape(-1) for c in challenges]))
        d_ch = torch.from_numpy(flat.view(np.int64)).to(dev)
    return d_pts, d_sc, d_ch


def _run_gm(torch, bv, recs, scs, ms, group, seed=1, challenges=None, weights=None, index_base=0):
    """the grouped check over a mixed batch -> (verdicts (count,) u32 in caller order, failed, redone).  weights: None (the
    key form, key from `seed`) or (count, 2) u64, caller order."""
    dev = torch.device("cuda:0")
    count = len(ms)
    d_pts, d_sc, d_ch = _upload(torch, bv, recs, scs, challenges)
    d_ok = torch.full((count,), 7, dtype=torch.int32, device=dev)
    d_w = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.uint64).view(np.int64)).to(dev) if weights is not None else None
    wsb = bv.grouped_mixed_workspace_bytes(ms, group)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    failed, redone = bv.run_grouped_mixed_device(d_pts.data_ptr(), d_sc.data_ptr(), ms, None if weights is not None else _key(seed),
                                                 index_base, d_ok.data_ptr(), d_ws.data_ptr(), wsb, group=group,
                                                 stream=torch.cuda.current_stream().cuda_stream,
                                                 d_challenges=d_ch.data_ptr() if d_ch is not None else 0,
                                                 d_weights=d_w.data_ptr() if d_w is not None else 0)
    torch.cuda.synchronize()
    return d_ok.cpu().numpy().astype(np.uint32), failed, redone


def _both(torch, bv, recs, scs, ms, group, tag, **kw):
    """the exact mixed call and the grouped one on the same input: equal vectors, predicted stats -> the vector"""
    exact, _ = _run_mixed(torch, bv, recs, scs, ms, challenges=kw.get("challenges"), want_result=False)
    got, failed, redone = _run_gm(torch, bv, recs, scs, ms, group, **kw)
    want = _predict(ms, group, exact)
    print(tag, "group", group, "count", len(ms), "rejected", int((exact != 0).sum()), "stats", (failed, redone), "predicted", want)
    assert got.tolist() == exact.tolist(), (tag, group, np.flatnonzero(got != exact).tolist())
    assert (failed, redone) == want, (tag, group, (failed, redone), want)
    return exact


def _verifier(B, cname, cps=None):
    cps = cps or _corpora(cname)
    cap = cps[CAP]
    a = B.Arith(cname)
    return a, B.BatchVerifier(B.PublicKey.from_points(a, cap.gh, cap.G, cap.H), N, CAP, window_bits=WB)


def _valid_proofs(B, a, cname, cps, m, distinct):
    """`distinct` valid proofs of shape (N, m) under the prefix key: oracle-made (device-proved on edwards25519, which the C
    oracle does not have) -> (records (distinct, NV, PW), scalars (distinct, 3, 4))"""
    vals = [[(41 * t + 13 * j + m) % (1 << N) for j in range(m)] for t in range(distinct)]
    gams = [[3 + 5 * t + j for j in range(m)] for t in range(distinct)]
    cp = cps[m]
    if cname == "ed25519":
        ded = B.BatchVerifier(B.PublicKey.from_points(a, cp.gh, cp.G, cp.H), N, m, window_bits=WB)
        pts, sc, V = ded.prove_batch(vals, gams)
        ded.close()
        return np.concatenate([pts, V], axis=1), sc
    out = []
    for t in range(distinct):
        pts, sc, V = O.range_prove(cp.opk, N, vals[t], gams[t])
        assert O.range_verify(cp.opk, N, m, pts, sc, V) == 0
        out.append((np.concatenate([pts, V]), np.array(sc, copy=True)))
    return np.stack([r for r, _ in out]), np.stack([s for _, s in out])


# ---- 1. the adversarial corpus, three curves ------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_grouped_mixed_corpus(cname):
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cps = _corpora(cname)
    a, bv = _verifier(B, cname)
    # wrong-round-count cases have no packed record (as in tests/test_gpu_mixed.py); the weighted checks assume prime-order
    # points modulo the identity class, so edwards25519 torsion stays out of them (as in tests/test_gpu_verdict_parity.py)
    # and nothing else does: BLS12-381 runs with the subgroup check on, the condition the header states
    cases = {}
    for m in CLASSES:
        rep = [c for c in cps[m].cases if c.k_ok]
        cases[m] = [c for c in rep if not (cname == "ed25519" and c.shifted)]
        dropped = [c for c in rep if c not in cases[m]]
        print(cname, m, "cases", len(cases[m]), "left out", [c.name for c in dropped])
        assert len(dropped) <= 3 and all(c.shifted for c in dropped), (cname, m, dropped)
        assert cname == "ed25519" or not dropped
    settings = (True,) if cname == "bls12_381" else (True, False)
    for order in ((1, 2, 4), (2, 4, 1), (4, 1, 2)):
        seq = _interleave(cases, order)
        recs = [_record(cases[m][i]) for m, i in seq]
        scs = np.stack([cases[m][i].sc for m, i in seq])
        ms = [m for m, _ in seq]
        for check in settings:
            bv.set_subgroup_check(check)
            for group in (2, 4, 8, 32):
                exact = _both(torch, bv, recs, scs, ms, group, (cname, order, check), seed=group)
                assert 0 in exact and 1 in exact
    bv.set_subgroup_check(False)
    bv.close()


# ---- 2. mostly valid blocks, groups across class boundaries -----------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_grouped_mixed_valid_blocks_and_one_tampered_proof(cname):
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cps = _corpora(cname)
    a, bv = _verifier(B, cname)
    bv.set_subgroup_check(cname == "bls12_381")
    counts = {1: 3, 2: 5, 4: 2}       # at group 4: group 0 holds three m = 1 proofs and one m = 2 proof, group 2 is short
    pool = {m: _valid_proofs(B, a, cname, cps, m, counts[m]) for m in CLASSES}
    rng = np.random.default_rng(3)
    order = [int(x) for x in rng.permutation(sum(counts.values()))]
    flat = [(m, t) for m in CLASSES for t in range(counts[m])]
    seq = [flat[i] for i in order]                                   # callers shuffled
    ms = [m for m, _ in seq]
    recs = [pool[m][0][t] for m, t in seq]
    scs = np.stack([pool[m][1][t] for m, t in seq])
    count = len(ms)
    g4 = B.mixed_groups(ms, 4)
    assert sorted(ms[i] for i in range(count) if g4[i] == 0) == [1, 1, 1, 2] and int((g4 == 2).sum()) == 2
    for group in (2, 4, 8, 16, 32):
        exact = _both(torch, bv, recs, scs, ms, group, (cname, "valid"), seed=group)
        assert exact.tolist() == [0] * count
        got, failed, redone = _run_gm(torch, bv, recs, scs, ms, group, seed=100 + group)
        assert got.tolist() == [0] * count and (failed, redone) == (0, 0)
    # each position in turn: r', s' or delta'
    for group in (2, 4, 32):
        g = B.mixed_groups(ms, group)
        for j in range(count):
            bad = scs.copy()
            bad[j, j % 3, 0] ^= np.uint64(1 + j)
            exact = _both(torch, bv, recs, bad, ms, group, (cname, "tampered", j), seed=7 * group + j)
            assert exact.tolist() == [1 if i == j else 0 for i in range(count)]
            got, failed, redone = _run_gm(torch, bv, recs, bad, ms, group, seed=j)
            assert (failed, redone) == (1, int((g == g[j]).sum())), (group, j)
    # a proof point exchanged for another, and a point that is not on the curve (fails its group whatever the weights)
    for j, what in ((1, "exchanged"), (count - 2, "off curve")):
        r2 = [np.array(r, copy=True) for r in recs]
        if what == "exchanged":
            r2[j][3] = recs[j][4]
        else:
            r2[j][0, 0] ^= np.uint64(1)
        for group in (4, 8):
            exact = _both(torch, bv, r2, scs, ms, group, (cname, what), seed=5)
            assert exact.tolist() == [1 if i == j else 0 for i in range(count)]
    bv.set_subgroup_check(False)
    bv.close()


# ---- 3. one class only ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_grouped_mixed_single_class(cname):
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cps = _corpora(cname)
    a, bv = _verifier(B, cname)
    bv.set_subgroup_check(cname == "bls12_381")
    count = 21
    for m in CLASSES:
        r, s = _valid_proofs(B, a, cname, cps, m, 7)
        recs = np.stack([r[i % 7] for i in range(count)])
        scs = np.stack([s[i % 7] for i in range(count)])
        for victims in ([], [0], [5, 6, 20]):
            bad = scs.copy()
            for t, v in enumerate(victims):
                bad[v, t % 3, 0] ^= np.uint64(2 + t)
            for group in (4, 8):
                exact = _both(torch, bv, list(recs), bad, [m] * count, group, (cname, "only", m), seed=group)
                assert exact.tolist() == [1 if i in victims else 0 for i in range(count)]
                if m == CAP:      # the capacity class alone: the grouped check of the same verifier, verdicts and stats
                    ok, failed, redone = run_grouped_device(torch, bv, recs, bad, group, seed=group)
                    got, f2, r2 = _run_gm(torch, bv, list(recs), bad, [m] * count, group, seed=group)
                    assert got.tolist() == ok.tolist() and (f2, r2) == (failed, redone)
    bv.set_subgroup_check(False)
    bv.close()


# ---- 4. Horner forms and exact slices -----------------------------------------------------------------------------------
def test_grouped_mixed_every_horner_form_and_exact_slices():
    """Two classes mixed; more groups than the tree Horner serves (G > 256: eight lanes per group; then, in the thousands, one
    lane per group), and more failing proofs in ONE class than one slice of the exact pass (2 048)."""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cname, cap_m = "bls12_381", 2
    cid = O.CURVE_IDS[cname]
    a = B.Arith(cname)
    opk = {m: O.PublicKey(cid, N * m) for m in (1, 2)}
    bv = B.BatchVerifier(B.PublicKey.from_points(a, opk[2].gh, opk[2].G, opk[2].H), N, cap_m, window_bits=5)
    bv.set_subgroup_check(True)
    base = {}
    for m in (1, 2):
        out = []
        for t in range(5):
            pts, sc, V = O.range_prove(opk[m], N, [(200 + 31 * t + j) % 256 for j in range(m)], [3 + t + j for j in range(m)])
            out.append((np.concatenate([pts, V]), np.array(sc, copy=True)))
        base[m] = out
    rng = np.random.RandomState(5)
    for count, group, nbad, share1 in ((1200, 2, 9, 0.5), (20480, 2, 40, 0.3), (6000, 2, 2500, 0.67)):
        ms = [1 if x < share1 else 2 for x in rng.rand(count)]
        pick = rng.randint(0, 5, size=count)
        recs = [base[m][i][0] for m, i in zip(ms, pick)]
        scs = np.stack([base[m][i][1] for m, i in zip(ms, pick)])
        if nbad > 2048:    # nearly all of them in class 1: one class's exact pass takes two slices
            ones = [i for i in range(count) if ms[i] == 1]
            victims = sorted(rng.choice(ones, size=nbad - 200, replace=False).tolist() +
                             rng.choice([i for i in range(count) if ms[i] == 2], size=200, replace=False).tolist())
        else:
            victims = sorted(rng.choice(count, size=nbad, replace=False).tolist())
        for v in victims:
            scs[v, 2, 0] ^= np.uint64(2)
        exact = _both(torch, bv, recs, scs, ms, group, ("horner", count), seed=count)
        assert int(exact.sum()) == nbad and all(exact[v] == 1 for v in victims)
        if nbad > 2048:
            g = B.mixed_groups(ms, group)
            hit = set(g[exact != 0].tolist())
            assert sum(1 for i in range(count) if ms[i] == 1 and g[i] in hit) > 2048
    bv.close()


def test_grouped_mixed_exact_slices_with_caller_challenges():
    """The exact pass's SECOND slice of one class with the caller's challenges present: the slice's challenge blocks are
    gathered with the class's own row length (3 + k_i scalars).  Device-proved transcript proofs of two classes, tiled; more
    tampered proofs in class 1 than one slice (2 048) and a few in class 2."""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cname, cap_m, count, group, nbad = "bls12_381", 2, 6000, 2, 2500
    opk = O.PublicKey(O.CURVE_IDS[cname], N * cap_m)
    bv = B.BatchVerifier(B.PublicKey.from_points(B.Arith(cname), opk.gh, opk.G, opk.H), N, cap_m, window_bits=5)
    bv.set_subgroup_check(True)
    sizes = [1, 2] * 5
    brecs, bsc = bv.prove_batch_mixed([[(200 + 31 * t + j) % 256 for j in range(m)] for t, m in enumerate(sizes)],
                                      [[3 + t + j for j in range(m)] for t, m in enumerate(sizes)], transcript=True)
    base = {m: [t for t in range(len(sizes)) if sizes[t] == m] for m in (1, 2)}
    rng = np.random.RandomState(11)
    ms = [1 if x < 0.67 else 2 for x in rng.rand(count)]
    pick = [base[m][i] for m, i in zip(ms, rng.randint(0, 5, size=count))]
    recs = [brecs[t] for t in pick]
    scs = np.stack([bsc[t] for t in pick])
    victims = sorted(rng.choice([i for i in range(count) if ms[i] == 1], size=nbad - 200, replace=False).tolist() +
                     rng.choice([i for i in range(count) if ms[i] == 2], size=200, replace=False).tolist())
    for v in victims:
        scs[v, 2, 0] ^= np.uint64(2)
    d_pts, _, _ = _upload(torch, bv, recs, scs)
    nch = [3 + (N * m).bit_length() - 1 for m in ms]
    d_ch = torch.zeros(sum(nch) * 4, dtype=torch.int64, device=torch.device("cuda:0"))
    wsb = bv.mixed_workspace_bytes(ms)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=torch.device("cuda:0"))
    bv.derive_challenges_mixed_device(d_pts.data_ptr(), ms, d_ch.data_ptr(), d_ws.data_ptr(), wsb,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    off = np.concatenate([[0], np.cumsum(nch)]).astype(int)
    flat = d_ch.cpu().numpy().view(np.uint64).reshape(-1, 4)
    ch = [flat[off[i]:off[i + 1]] for i in range(count)]
    exact = _both(torch, bv, recs, scs, ms, group, "challenges, two slices", seed=count, challenges=ch)
    assert int(exact.sum()) == nbad and all(exact[v] == 1 for v in victims)
    g = B.mixed_groups(ms, group)
    hit = set(g[exact != 0].tolist())
    assert sum(1 for i in range(count) if ms[i] == 1 and g[i] in hit) > 2048
    bv.close()


# ---- 5. transcript ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_grouped_mixed_transcript(cname):
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cps = _corpora(cname, True)
    a, bv = _verifier(B, cname, cps)
    bv.set_subgroup_check(cname == "bls12_381")
    cases = {m: list(cps[m].cases) for m in CLASSES}
    seq = _interleave(cases, (4, 1, 2))
    recs = [_record(cases[m][i]) for m, i in seq]
    scs = np.stack([cases[m][i].sc for m, i in seq])
    ms = [m for m, _ in seq]
    d_pts, _, _ = _upload(torch, bv, recs, scs)
    nch = [3 + (N * m).bit_length() - 1 for m in ms]
    d_ch = torch.zeros(sum(nch) * 4, dtype=torch.int64, device=torch.device("cuda:0"))
    wsb = bv.mixed_workspace_bytes(ms)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=torch.device("cuda:0"))
    bv.derive_challenges_mixed_device(d_pts.data_ptr(), ms, d_ch.data_ptr(), d_ws.data_ptr(), wsb,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flat = d_ch.cpu().numpy().view(np.uint64)
    ch, off = [], 0
    for k in nch:
        ch.append(flat[off * 4:(off + k) * 4].reshape(k, 4))
        off += k
    for group in (2, 4, 8):
        exact = _both(torch, bv, recs, scs, ms, group, (cname, "transcript"), seed=group, challenges=ch)
        assert exact.tolist() == [cases[m][i].expect for m, i in seq] and 0 in exact and 1 in exact
    # valid proofs only, then one of them tampered
    valid = [j for j, (m, i) in enumerate(seq) if cases[m][i].expect == 0]
    assert len(valid) >= 6
    vrecs, vms, vch = [recs[j] for j in valid], [ms[j] for j in valid], [ch[j] for j in valid]
    vscs = scs[valid]
    exact = _both(torch, bv, vrecs, vscs, vms, 4, (cname, "transcript valid"), seed=1, challenges=vch)
    assert exact.tolist() == [0] * len(valid)
    bad = vscs.copy()
    bad[len(valid) // 2, 0, 0] ^= np.uint64(4)
    exact = _both(torch, bv, vrecs, bad, vms, 4, (cname, "transcript tampered"), seed=2, challenges=vch)
    assert exact.tolist() == [1 if j == len(valid) // 2 else 0 for j in range(len(valid))]
    # without the challenges the transcript's proofs fail under the literal ones: every group fails, and the vector still
    # equals the exact call's
    exact = _both(torch, bv, vrecs, vscs, vms, 4, (cname, "no challenges"), seed=3)
    assert exact.tolist() == [1] * len(valid)
    got, failed, redone = _run_gm(torch, bv, vrecs, vscs, vms, 4, seed=3)
    assert (failed, redone) == ((len(valid) + 3) // 4, len(valid))
    bv.set_subgroup_check(False)
    bv.close()


# ---- 6. weights -----------------------------------------------------------------------------------------------------------
def test_grouped_mixed_weights_belong_to_the_callers():
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cname = "secp256k1"
    cps = _corpora(cname)
    a, bv = _verifier(B, cname)
    pool = {m: _valid_proofs(B, a, cname, cps, m, 4) for m in CLASSES}
    seq = [(2, 0), (1, 0), (4, 0), (1, 1), (2, 1), (4, 1), (1, 2), (2, 2), (1, 3), (4, 2), (2, 3)]
    ms = [m for m, _ in seq]
    count = len(ms)
    recs = [pool[m][0][t] for m, t in seq]
    scs = np.stack([pool[m][1][t] for m, t in seq])
    scs[4, 1, 0] ^= np.uint64(1)
    scs[8, 2, 0] ^= np.uint64(6)
    rng = np.random.default_rng(9)
    weights = rng.integers(1, 1 << 62, size=(count, 2), dtype=np.uint64)
    for group in (2, 4):
        exact = _both(torch, bv, recs, scs, ms, group, "key form", seed=group, index_base=1 << 40)
        assert exact.tolist() == [1 if i in (4, 8) else 0 for i in range(count)]
        _both(torch, bv, recs, scs, ms, group, "weight buffer", weights=weights)
        # the callers permuted together with their weights: the verdicts permuted
        perm = [int(x) for x in rng.permutation(count)]
        got, failed, redone = _run_gm(torch, bv, [recs[i] for i in perm], scs[perm], [ms[i] for i in perm], group,
                                      weights=weights[perm])
        assert got.tolist() == [int(exact[i]) for i in perm]
        assert (failed, redone) == _predict([ms[i] for i in perm], group, got)
    # WHICH weight a caller gets, pinned by the failure the header warns of: two copies of one proof whose delta' are moved by
    # +1 and -1 (delta' enters the MulVec linearly, in h's scalar alone) cancel in a group that gives both the SAME weight,
    # and only then
    r1, s1 = pool[1][0][0], pool[1][1][0]
    up, down = s1.copy(), s1.copy()
    d = int(s1[2, 0])
    assert 0 < d < (1 << 64) - 1
    up[2, 0], down[2, 0] = np.uint64(d + 1), np.uint64(d - 1)
    ms2 = [2, 1, 4, 1, 2]            # callers 1 and 3 are gathered positions 0 and 1: one group at any group size
    recs2 = [pool[2][0][0], r1, pool[4][0][0], r1, pool[2][0][1]]
    scs2 = np.stack([pool[2][1][0], up, pool[4][1][0], down, pool[2][1][1]])
    exact, _ = _run_mixed(torch, bv, recs2, scs2, ms2, want_result=False)
    assert exact.tolist() == [0, 1, 0, 1, 0]
    w = rng.integers(1, 1 << 62, size=(5, 2), dtype=np.uint64)
    got, failed, redone = _run_gm(torch, bv, recs2, scs2, ms2, 2, weights=w)
    assert got.tolist() == [0, 1, 0, 1, 0] and (failed, redone) == (1, 2)
    same = w.copy()
    same[3] = same[1]                # caller order: the two copies share a weight, the group's sum is the identity
    got, failed, redone = _run_gm(torch, bv, recs2, scs2, ms2, 2, weights=same)
    assert got.tolist() == [0, 0, 0, 0, 0] and (failed, redone) == (0, 0)
    other = w.copy()
    other[2] = other[1]              # the same weight on another caller (gathered positions 0 and 4): no cancellation
    got, failed, redone = _run_gm(torch, bv, recs2, scs2, ms2, 2, weights=other)
    assert got.tolist() == [0, 1, 0, 1, 0] and (failed, redone) == (1, 2)
    bv.close()


# ---- 7. the headline shape ----------------------------------------------------------------------------------------------
def test_grouped_mixed_big_shape():
    """capacity (64, 16) at window 8 on BLS12-381: the 4 096 x (64,1) + 256 x (64,16) device-proved block of
    test_mixed_big_shape, shuffled, five tampered, group 32"""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cname, n, M = "bls12_381", 64, 16
    big = VC.corpus(cname, n, M)
    a = B.Arith(cname)
    bv = B.BatchVerifier(B.PublicKey.from_points(a, big.gh, big.G, big.H), n, M, window_bits=8)
    e1 = B.BatchVerifier(B.PublicKey.from_points(a, big.gh, big.G[:n], big.H[:n]), n, 1, window_bits=8)
    bv.set_subgroup_check(True)
    rng = np.random.default_rng(7)
    p1, s1, V1 = e1.prove_batch(rng.integers(0, 1 << 31, size=(4096, 1), dtype=np.uint64).tolist(),
                                [[int(x)] for x in rng.integers(1, 1 << 62, size=4096)])
    p16, s16, V16 = bv.prove_batch(rng.integers(0, 1 << 31, size=(256, M), dtype=np.uint64).tolist(),
                                   [[int(x) for x in row] for row in rng.integers(1, 1 << 62, size=(256, M))])
    e1.close()
    r1 = np.concatenate([p1, V1], axis=1)
    r16 = np.concatenate([p16, V16], axis=1)
    order = rng.permutation(4096 + 256)
    ms = [1 if i < 4096 else M for i in order]

    def block():
        return ([r1[i] if i < 4096 else r16[i - 4096] for i in order],
                np.stack([s1[i] if i < 4096 else s16[i - 4096] for i in order]))
    recs, scs = block()
    exact = _both(torch, bv, recs, scs, ms, 32, "big valid", seed=1)
    assert not exact.any()
    for t in (3, 1000, 4095):
        s1[t, 1, 0] ^= 1
    for t in (0, 200):
        s16[t, 1, 0] ^= 1
    recs, scs = block()
    exact = _both(torch, bv, recs, scs, ms, 32, "big tampered", seed=2)
    assert int(exact.sum()) == 5
    assert sorted(int(order[j]) for j in np.flatnonzero(exact)) == [3, 1000, 4095, 4096, 4296]
    bv.close()


# ---- 8. arguments -----------------------------------------------------------------------------------------------------------
def test_grouped_mixed_arguments():
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cname = "secp256k1"
    cps = _corpora(cname)
    a, bv = _verifier(B, cname)
    good = [next(c for c in cps[m].cases if c.k_ok and c.expect == 0) for m in CLASSES]
    recs = [_record(c) for c in good]
    scs = np.stack([c.sc for c in good])
    dev = torch.device("cuda:0")
    d_pts, d_sc, _ = _upload(torch, bv, recs, scs)
    d_ok = torch.full((3,), 7, dtype=torch.int32, device=dev)
    ms = list(CLASSES)
    wsb = bv.grouped_mixed_workspace_bytes(ms, 2)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    key = _key(0)

    def call(ms_, group, ws_bytes=wsb):
        return bv.run_grouped_mixed_device(d_pts.data_ptr(), d_sc.data_ptr(), ms_, key, 0, d_ok.data_ptr(), d_ws.data_ptr(),
                                           ws_bytes, group=group, stream=st)
    for bad_ms, where in (([1, 3, 4], 1), ([1, 2, 2 * CAP], 2), ([0, 2, 4], 0)):
        assert bv.grouped_mixed_workspace_bytes(bad_ms, 2) == 0
        assert bv.serialized_grouped_mixed_workspace_bytes(bad_ms, 2) == 0
        with pytest.raises(B.BppError) as ei:
            call(bad_ms, 2)
        assert ei.value.code == -1 and ("m_of[%d]" % where) in str(ei.value), str(ei.value)
    for group in (0, 1, 3, 12):
        assert bv.grouped_mixed_workspace_bytes(ms, group) == 0
        assert bv.serialized_grouped_mixed_workspace_bytes(ms, group) == 0
        with pytest.raises(B.BppError) as ei:
            call(ms, group)
        assert ei.value.code == -1 and "group" in str(ei.value), str(ei.value)
    with pytest.raises(B.BppError) as ei:
        call(ms, 2, wsb - 1)
    assert ei.value.code == -1 and "workspace" in str(ei.value)
    with pytest.raises(B.BppError):      # neither a key nor a weight buffer
        B._lib.check(B._lib.lib().bpp_verifier_run_grouped_mixed(
            bv.handle, d_pts.data_ptr(), d_sc.data_ptr(), bv._ms(ms).ctypes.data, 3, None, None, 0, None, 2, d_ok.data_ptr(),
            None, d_ws.data_ptr(), wsb, None), "weights")
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [7, 7, 7]
    assert call([], 2) == (0, 0)                                      # an empty batch
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [7, 7, 7]
    assert call(ms, 2) == (0, 0)
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [0, 0, 0]
    bv.close()


# ---- 9. behind the decoder ----------------------------------------------------------------------------------------------
def _run_sgm(torch, bv, blobs, comms, ms, group, seed=1, transcript=False, uncompressed=False, index_base=0):
    dev = torch.device("cuda:0")
    count = len(ms)
    d_p = torch.from_numpy(_u8(blobs)).to(dev)
    d_c = torch.from_numpy(_u8(comms)).to(dev)
    d_ok = torch.full((count,), 7, dtype=torch.int32, device=dev)
    wsb = bv.serialized_grouped_mixed_workspace_bytes(ms, group)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    stats = bv.verify_serialized_grouped_mixed_device(d_p.data_ptr(), d_c.data_ptr(), ms, d_ok.data_ptr(), d_ws.data_ptr(), wsb,
                                                      _key(seed), index_base, group, torch.cuda.current_stream().cuda_stream,
                                                      transcript=transcript, uncompressed=uncompressed)
    torch.cuda.synchronize()
    return d_ok.cpu().numpy().astype(np.uint32), stats


def _both_serialized(torch, bv, blobs, comms, ms, group, tag, **kw):
    exact = _run_serialized_mixed(torch, bv, blobs, comms, ms, transcript=kw.get("transcript", False),
                                  uncompressed=kw.get("uncompressed", False))
    got, stats = _run_sgm(torch, bv, blobs, comms, ms, group, **kw)
    want = _predict(ms, group, exact)
    print(tag, "group", group, "count", len(ms), "statuses", np.bincount(exact, minlength=3).tolist(), "stats", stats,
          "predicted", want)
    assert got.tolist() == exact.tolist(), (tag, group, np.flatnonzero(got != exact).tolist())
    assert stats == want, (tag, group, stats, want)
    return exact


@pytest.mark.parametrize("cname", CURVES)
def test_serialized_grouped_mixed_corpus(cname):
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cps = _corpora(cname)
    a, bv = _verifier(B, cname)
    # every case with a container encoding (the builder of tests/test_gpu_serialized_mixed.py); the decoder's subgroup test
    # rejects what the weighted check could not take, so no case is left out here
    cases = {m: [c for c in cps[m].cases if c.status is not None] for m in CLASSES}
    for version in ((1, 2) if cname != "ed25519" else (1,)):
        enc = {m: [VC.encode_case(cps[m], c, version) for c in cases[m]] for m in CLASSES}
        for order in ((1, 2, 4), (4, 1, 2)):
            seq = _interleave(cases, order)
            ms = [m for m, _ in seq]
            blobs, comms = [enc[m][i][0] for m, i in seq], [enc[m][i][1] for m, i in seq]
            for group in (2, 4, 32):
                exact = _both_serialized(torch, bv, blobs, comms, ms, group, (cname, version, order), seed=group,
                                         uncompressed=version == 2)
                assert exact.tolist() == [cases[m][i].status for m, i in seq]
                assert {0, 1} <= set(exact.tolist()) and (2 in exact or cname == "secp256k1")
    bv.close()


@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_serialized_grouped_mixed_transcript(cname):
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cps = _corpora(cname, True)
    a, bv = _verifier(B, cname, cps)
    cases = {m: list(cps[m].cases) for m in CLASSES}
    status = {m: [cps[m].container_status(c) for c in cases[m]] for m in CLASSES}
    assert all(s is not None for m in CLASSES for s in status[m])
    for version in (1, 2):
        enc = {m: [VC.encode_case(cps[m], c, version) for c in cases[m]] for m in CLASSES}
        seq = _interleave(cases, (4, 1, 2))
        ms = [m for m, _ in seq]
        blobs, comms = [enc[m][i][0] for m, i in seq], [enc[m][i][1] for m, i in seq]
        for group in (2, 8):
            exact = _both_serialized(torch, bv, blobs, comms, ms, group, (cname, "transcript", version), seed=group,
                                     transcript=True, uncompressed=version == 2)
            assert exact.tolist() == [status[m][i] for m, i in seq]
    # the transcript binds the proof: with the literal challenges the valid proofs fail, here as on the exact path
    exact = _both_serialized(torch, bv, blobs, comms, ms, 4, (cname, "literal challenges"), seed=4, uncompressed=True)
    assert 0 not in exact
    bv.close()


@pytest.mark.parametrize("cname", CURVES)
def test_serialized_grouped_mixed_format_error_is_local(cname):
    """one corrupted container at a time in an all-valid interleaved batch: exactly that proof reads 2, no other status moves,
    and its group counts as failed"""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    cps = _corpora(cname)
    a, bv = _verifier(B, cname)
    cases = {m: [c for c in cps[m].cases if c.status == 0][:5] for m in CLASSES}
    assert all(len(cases[m]) >= 4 for m in CLASSES)
    enc = {m: [VC.encode_case(cps[m], c) for c in cases[m]] for m in CLASSES}
    seq = _interleave(cases, (2, 4, 1))
    ms = [m for m, _ in seq]
    count = len(ms)
    blobs, comms = [enc[m][i][0] for m, i in seq], [enc[m][i][1] for m, i in seq]
    for group in (4, 32):
        got, stats = _run_sgm(torch, bv, blobs, comms, ms, group)
        assert got.tolist() == [0] * count and stats == (0, 0)
    targets = {0, count - 1}
    for m in CLASSES:
        pos = [j for j, mm in enumerate(ms) if mm == m]
        targets |= {pos[0], pos[-1]}
    r_le = cps[CAP].r.to_bytes(32, "little")
    g = B.mixed_groups(ms, 4)
    for j in sorted(targets):
        blob = blobs[j]
        other = next(x for x in CLASSES if x != ms[j])
        for what, bad in (("m", blob[:7] + bytes([other]) + blob[8:]), ("scalar = r", blob[:-32] + r_le),
                          ("flags", blob[:12] + bytes([{"bls12_381": blob[12] & 0x7f, "secp256k1": 4,
                                                        "ed25519": blob[12] | 1}[cname]]) + blob[13:])):
            assert bad != blob
            exact = _both_serialized(torch, bv, blobs[:j] + [bad] + blobs[j + 1:], comms, ms, 4, (cname, j, what), seed=j)
            assert exact.tolist() == [2 if t == j else 0 for t in range(count)], (j, what)
            got, stats = _run_sgm(torch, bv, blobs[:j] + [bad] + blobs[j + 1:], comms, ms, 4, seed=j)
            assert stats == (1, int((g == g[j]).sum()))
    bv.close()
