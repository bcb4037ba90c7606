"""-m gpu: the launch plan of k_fixed_msm (csrc/fixed_plan.hpp) where it engages -- long lanes for all proofs but the last
1024 -- on CHOSEN scalars and points, through bpp_debug_verifier_mulvec and the builders of tests/mulvec_cases.py.

The shapes of GPU_CASES have NF <= 514 and never meet the plan; these are the smallest that do.  n=64, m=8 is NF = 1026:
two blocks per proof, so a long lane takes G = 8 whole generators and the 2 left-over ones are spread; counts 1025 (ONE long
block in front of 2048 short ones), 1100, and 2100 (more long blocks than the chip holds at a time).  n=64, m=16 is NF =
2050, four blocks per proof and G = 16: the lane geometry of the headline pass.  Every case makes one call over the cycle
of record classes and then sweeps the single non-zero term -- scalar 1 and r - 1 -- over all N terms at the same count:
verdict and result point of EVERY record are held to the builder's big-integer answer, and the reported geometry to
[0, per].  A record runs in a long lane only at a position below long_count = count - 1024, so where that zone is wide
enough (count 2100 at m=8; count 3200 at m=16, a case added for this) the sweep's calls step by long_count and EVERY one-hot
record meets a long lane in some call as well as a short one: that pins lane -> generator -> table row for G = 8 and G = 16
term by term.  At 1025 and 1100 the long zone holds 1 and 76 positions; there the sweep localises a fault in the short zone
only, and the long lanes are held by the records of the cycle (random, all_one, ..), which do land in them.  At 1024 proofs
the plan is off, and the same records must give what they give at 1100.

The records are built once per shape and shared by its counts (a call takes its records by position, modulo their number)."""

import numpy as np
import pytest

import mulvec_cases as M
from gpu_util import need_gpu
from test_gpu_mulvec_backend import DISTINCT_PER_CLASS, _check, _hook

pytestmark = pytest.mark.gpu

RES = 1024
SHAPES_M8 = [("bls12_381", 64, 8, 7), ("bls12_381", 64, 8, 10), ("secp256k1", 64, 8, 9), ("ed25519", 64, 8, 7)]
# (curve, n, m, window_bits, count, blocks per proof)
CASES = [s + (count, 2) for s in SHAPES_M8 for count in (1025, 1100, 2100)] + [("bls12_381", 64, 16, 10, 1100, 4), ("bls12_381", 64, 16, 10, 3200, 4)]


def _case_id(t):
    return "%s-%dx%d-c%d-count%d" % t[:5]


@pytest.fixture(scope="module")
def world():
    """verifiers and record sets by (curve, n, m, window_bits), made on first use; the verifiers close with the module"""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    engines, records, ariths = {}, {}, {}

    def engine(shape):
        if shape not in engines:
            cname, n, m, c = shape
            a = ariths.setdefault(cname, B.Arith.init(cname))
            pk = B.PublicKey.new(a, n * m)
            gh, G, H = M.key_wire(cname, n * m)
            assert np.array_equal(pk.gh, gh) and np.array_equal(pk.G_vec, G) and np.array_equal(pk.H_vec, H)
            engines[shape] = B.BatchVerifier(pk, n, m, window_bits=c)
        return engines[shape]

    def material(shape):
        """(the cycle of record classes, the one-hot sweep of all N terms with both scalars)"""
        if shape not in records:
            cname, n, m, c = shape
            cl = M.classes_of(cname)
            cyc = M.batch(cname, n, m, c, DISTINCT_PER_CLASS * len(cl))
            assert set(cyc.cls) == set(cl)
            hot = M.batch(cname, n, m, c, 2 * cyc.shape.N, classes=("one_hot",))
            swept = {(hot.note[i], hot.scalars_int[i][hot.note[i]]) for i in range(len(hot.cls))}
            assert swept == {(t, s) for t in range(cyc.shape.N) for s in (1, cyc.shape.r - 1)}
            records[shape] = (cyc, hot)
        return records[shape]

    yield torch, engine, material
    for bv in engines.values():
        bv.close()


def _calls(cyc, hot, count):
    """(batch, the batch's record behind each record of the call): the cycle, then the sweep.  The sweep's calls step by
    count, or by the width of the long zone where two calls of that step cover the sweep: every one-hot record then sits
    below long_count in one of them"""
    longs = max(count - RES, 0)
    in_long = 2 * longs >= len(hot.cls)
    calls = [(cyc, np.arange(count) % len(cyc.cls))]
    for off in range(0, len(hot.cls), longs if in_long else count):
        calls.append((hot, (off + np.arange(count)) % len(hot.cls)))
    assert {int(i) for _, idx in calls[1:] for i in idx} == set(range(len(hot.cls)))
    if in_long:
        assert len(calls) == 3 and {int(i) for _, idx in calls[1:] for i in idx[:longs]} == set(range(len(hot.cls)))
    return calls


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_long_lanes_on_chosen_scalars_and_points(case, world):
    cname, n, m, c, count, per = case
    torch, engine, material = world
    sh = M.Shape(cname, n, m, c)
    assert sh.NF // (128 * 4) == per and count > RES        # the throughput bound sets per: the plan engages
    bv = engine(case[:4])
    cyc, hot = material(case[:4])
    calls = _calls(cyc, hot, count)
    assert (2 * (count - RES) >= len(hot.cls)) == (count in (2100, 3200))   # the sweeps that put every term into a long lane
    for b, idx in calls:
        ok, res, geo = _hook(torch, bv, 0, b.records[idx], b.scalars[idx])
        assert geo == [0, per], "launch geometry %s, the case names %s" % (geo, [0, per])
        _check(b, idx, ok, res, _case_id(case))


@pytest.mark.parametrize("shape", SHAPES_M8, ids=lambda t: "%s-%dx%d-c%d" % t)
def test_plan_off_at_1024_gives_what_1100_gives(shape, world):
    """1024 proofs are all short zone: no long block.  The same records, in the same positions, at 1100 -- where the first
    76 are long -- give the same verdicts and the same points."""
    torch, engine, material = world
    bv = engine(shape)
    cyc, hot = material(shape)
    for b, idx in _calls(cyc, hot, 1100)[:2]:
        ok_on, res_on, geo_on = _hook(torch, bv, 0, b.records[idx], b.scalars[idx])
        ok_off, res_off, geo_off = _hook(torch, bv, 0, b.records[idx[:RES]], b.scalars[idx[:RES]])
        assert geo_on == [0, 2] and geo_off == [0, 2]
        _check(b, idx[:RES], ok_off, res_off, "%s at 1024" % (shape,))
        assert np.array_equal(ok_off, ok_on[:RES]) and np.array_equal(res_off, res_on[:RES])
