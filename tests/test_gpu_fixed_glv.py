"""-m gpu: the fixed-generator MulVec through the shared GLV window tables (BLS12-381: csrc/kernels.hpp k_fixed_msm with
fixed_glv<C>(), two phases per lane and the endomorphism applied once to the accumulator).

Per shape: valid proofs from prove_batch plus a tampered subset must give the exact verdict vector, and the MulVec result
the verifier reports (d_out_result) must be the group element that the naive MulVec (bpp_msm_batch: one double-and-add per
term, no tables) computes from the same points with the scalars the verifier reports (d_out_scalars).  The shapes cover the
launch geometries: fewer generators than lanes, one / two / four blocks per proof, one, two and four generators per lane,
left-over generators in both phases, and window counts of both parities.  Also: the batched prover (ROLE 2, which walks the
same tables) against the single-proof prover, and the refusal of generators outside G1."""

import ctypes

import numpy as np
import pytest

from gpu_util import need_gpu, run_verifier_device

pytestmark = pytest.mark.gpu

DISTINCT = 32   # distinct proofs per shape; a batch repeats them (the verdicts of a batch do not depend on distinctness)


def _values(seed, m, nbits):
    vals = [(((0x9E3779B97F4A7C15 * (j + 1 + seed)) & 0xFFFFFFFFFFFFFFFF) % (1 << 31)) % (1 << nbits) for j in range(m)]
    return vals, [j + 3 + seed for j in range(m)]


def _batch(bv, n, m, count):
    d = min(DISTINCT, count)
    vg = [_values(17 * i + 1, m, n) for i in range(d)]
    pts, scs, V = bv.prove_batch([v for v, _ in vg], [g for _, g in vg])
    recs = np.ascontiguousarray(np.concatenate([pts, V], axis=1))
    idx = np.arange(count) % d
    return np.ascontiguousarray(recs[idx]), np.ascontiguousarray(scs[idx])


def _tamper(recs, scs, which):
    """bit flips in r' / s' / delta' and, every fourth, the A of a proof whose A differs"""
    rec_t, sc_t = recs.copy(), scs.copy()
    count = recs.shape[0]
    for j, i in enumerate(which):
        kind = j % 4
        if kind < 3:
            sc_t[i, kind, 0] ^= np.uint64(1 << (j % 60))
        else:
            src = next(s for s in range(i + 1, i + count) if not np.array_equal(recs[s % count, 0], recs[i, 0])) % count
            rec_t[i, 0] = recs[src, 0]
    return rec_t, sc_t


def _mulvec_points(pk, rec, n, m, k):
    """the points of the verification MulVec in the order of its scalars: head, g, h, L.., R.., G.., H.., V.."""
    head = rec[:3][::-1] if m == 1 else rec[:3]
    return np.concatenate([head, pk.gh, rec[3:3 + 2 * k], pk.G_vec[:n * m], pk.H_vec[:n * m], rec[3 + 2 * k:]])


@pytest.mark.parametrize("n,m,count,wb", [(8, 1, 3, 10), (64, 1, 2048, 13), (64, 2, 2048, 13), (64, 16, 2048, 10),
                                         (64, 16, 2048, 11)])
def test_verdicts_and_mulvec_result(n, m, count, wb):
    torch = need_gpu()
    import bulletproofsplus_amd as B
    a = B.Arith.init("bls12_381")
    pk = B.PublicKey.new(a, n * m)
    bv = B.BatchVerifier(pk, n, m, window_bits=wb)
    assert bv.table_bytes < 2 * 10**9
    k = bv.k
    recs, scs = _batch(bv, n, m, count)
    ok, _, res = run_verifier_device(torch, bv, recs, scs, want_scalars=False)
    assert ok.tolist() == [0] * count
    assert all(int(r[2 * a.L]) == 1 for r in res)                      # every MulVec result is the identity
    nbad = 1 if count < 8 else 61
    which = np.sort(np.random.RandomState(7 + wb).choice(count, size=nbad, replace=False))
    rec_t, sc_t = _tamper(recs, scs, which)
    ok, vsc, res = run_verifier_device(torch, bv, rec_t, sc_t)
    want = np.zeros(count, dtype=np.uint32)
    want[which] = 1
    assert np.array_equal(ok, want)
    # tampered proofs (a result that is not the identity, with every fixed generator's scalar changed by the tampering of
    # r', s' or delta') and two valid ones
    good = np.setdiff1d(np.arange(count), which)
    sample = [int(i) for i in which[:6]] + [int(i) for i in good[:2]]
    N = bv.msm_len
    pts = np.concatenate([_mulvec_points(pk, rec_t[i], n, m, k) for i in sample])
    naive = B.msm_batch(a, np.concatenate([vsc[i] for i in sample]), pts, [N] * len(sample))
    for i, want_pt in zip(sample, naive):
        assert np.array_equal(res[i], want_pt), i
        assert (int(res[i][2 * a.L]) == 1) == (i not in which)
    bv.close()


def test_batched_prover_matches_single_proofs():
    """ROLE 2 of the kernel (sparse virtual proofs, the +-1 scalars of range A, zero scalars) against RangeProof.prove"""
    need_gpu()
    import bulletproofsplus_amd as B
    n, m = 64, 2
    a = B.Arith.init("bls12_381")
    pk = B.PublicKey.new(a, n * m)
    bv = B.BatchVerifier(pk, n, m, window_bits=10)
    vg = [_values(5 * i + 2, m, n) for i in range(3)] + [([0, (1 << 31) - 1], [1, 2])]
    pts, scs, V = bv.prove_batch([v for v, _ in vg], [g for _, g in vg])
    for i, (vals, gams) in enumerate(vg):
        pr = B.RangeProver.new()
        for v, g in zip(vals, gams):
            pr.commit(pk, v, g)
        proof = B.RangeProof.prove(pk, n, pr)
        assert np.array_equal(pts[i], proof.points_wire()), i
        assert np.array_equal(scs[i], proof.scalars_wire()), i
        assert np.array_equal(V[i], np.asarray(pr.commitment_vec).reshape(V[i].shape)), i
    bv.close()


def test_generator_outside_g1_is_refused():
    """[z^2] P = (beta x, -y) holds on G1 only: P + (0, 2) is a curve point outside it ((0, 2) has order 3 on y^2 = x^3 + 4)"""
    need_gpu()
    import bulletproofsplus_amd as B
    from bulletproofsplus_amd import _lib as L
    n, m = 8, 1
    a = B.Arith.init("bls12_381")
    pk = B.PublicKey.new(a, n * m)
    T = np.zeros(a.PW, dtype=np.uint64)
    T[a.L] = 2
    bad = np.zeros(a.PW, dtype=np.uint64)
    G = np.ascontiguousarray(pk.G_vec).copy()
    vp = ctypes.c_void_p
    assert L.lib().bpp_debug_point_op(a.handle, 0, G[5].ctypes.data_as(vp), T.ctypes.data_as(vp), 1, bad.ctypes.data_as(vp)) == 0
    G[5] = bad
    B.BatchVerifier(B.PublicKey.from_points(a, pk.gh, pk.G_vec, pk.H_vec), n, m, window_bits=6).close()   # the key itself is fine
    with pytest.raises(B.BppError) as e:
        B.BatchVerifier(B.PublicKey.from_points(a, pk.gh, G, pk.H_vec), n, m, window_bits=6)
    assert e.value.code == -1 and "subgroup" in str(e.value)
