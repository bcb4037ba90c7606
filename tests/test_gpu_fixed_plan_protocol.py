"""-m gpu: real range proofs through BatchVerifier.run_device at a shape where the launch plan of k_fixed_msm engages
(csrc/fixed_plan.hpp): n=64, m=8 (NF = 1026, two blocks per proof), 1100 proofs -- the first 76 take one long block each,
the last 1024 two short ones.  Sixteen distinct proofs of the batched prover, eight of them tampered (bit flips in r', s',
delta', one A exchanged for another proof's), tiled to 1100 so that valid and tampered records fall into both zones.  The
verdict vector is exact, the valid records' MulVec is the point at infinity, the untiled sixteen agree with the CPU oracle,
and verdicts and result points are identical to the same records run as two calls of 550, where the plan is off."""

import numpy as np
import pytest

import oracle as O
from gpu_util import need_gpu, run_verifier_device

pytestmark = pytest.mark.gpu

N_BITS, M, C, DISTINCT, COUNT = 64, 8, 7, 16, 1100
# base record -> (scalar row: 0 r', 1 s', 2 delta'; limb; bit), or "A": its A is the next proof's
TAMPER = {1: (0, 0, 0), 3: (0, 3, 20), 4: (1, 1, 17), 6: (1, 2, 1), 9: (2, 0, 5), 10: (2, 3, 40), 12: (2, 1, 63), 15: "A"}


def test_real_proofs_in_both_zones_match_the_unplanned_launch():
    torch = need_gpu()
    import bulletproofsplus_amd as B
    a = B.Arith.init("bls12_381")
    pk = B.PublicKey.new(a, N_BITS * M)
    eng = B.BatchVerifier(pk, N_BITS, M, window_bits=C)
    rnd = np.random.RandomState(6408)
    vals = rnd.randint(0, 2**31 - 1, size=(DISTINCT, M)).astype(np.uint64)
    gams = [[int(x) for x in row] for row in rnd.randint(1, 2**62, size=(DISTINCT, M))]
    pts, sc, V = eng.prove_batch(vals, gams)
    assert len({pts[i].tobytes() for i in range(DISTINCT)}) == DISTINCT
    recs = np.ascontiguousarray(np.concatenate([pts, V], axis=1))
    sc = np.ascontiguousarray(sc).copy()
    for i, how in TAMPER.items():
        if how == "A":
            recs[i, 0] = pts[(i + 1) % DISTINCT, 0]
        else:
            row, limb, bit = how
            sc[i, row, limb] ^= np.uint64(1) << np.uint64(bit)
    want = np.array([1 if i in TAMPER else 0 for i in range(DISTINCT)], dtype=np.uint32)
    assert len(TAMPER) == 8
    # the sixteen against the CPU oracle: verdict and MulVec result
    opk = O.PublicKey(O.BLS12_381, N_BITS * M)
    nrec = pts.shape[1]
    ok16, _, res16 = run_verifier_device(torch, eng, recs, sc, want_scalars=False)
    assert ok16.tolist() == want.tolist()
    for i in range(DISTINCT):
        rc, _, exp = O.range_verify(opk, N_BITS, M, recs[i, :nrec], sc[i], recs[i, nrec:], want_result=True)
        assert rc == want[i] and np.array_equal(res16[i], exp), i
    # tiled to 1100: the plan engages (blocks per proof stays 2: the short zone's)
    idx = np.arange(COUNT) % DISTINCT
    big_recs, big_sc = recs[idx], sc[idx]
    eng.set_profiling(True)
    ok, _, res = run_verifier_device(torch, eng, big_recs, big_sc, want_scalars=False)
    assert eng.profile()[2] == 2
    eng.set_profiling(False)
    assert ok.tolist() == want[idx].tolist()
    assert np.array_equal(res, res16[idx])
    assert all(a.is_zero(res[i]) for i in range(COUNT) if not want[idx[i]])
    # ... and as two calls of 550, where it does not
    half = COUNT // 2
    for lo in (0, half):
        ok_h, _, res_h = run_verifier_device(torch, eng, big_recs[lo:lo + half], big_sc[lo:lo + half], want_scalars=False)
        assert np.array_equal(ok_h, ok[lo:lo + half]) and np.array_equal(res_h, res[lo:lo + half]), lo
    eng.close()
