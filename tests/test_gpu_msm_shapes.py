"""-m gpu: the bucket-method MulVec (csrc/pippenger.hpp behind bpp_msm_device, bpp_msm_pippenger and bpp_msm from n = 4096
up) in every regime of its shape: chunk lengths 16, 32 and 64 (the entry ring of k_pip_chunks cycling through its two
slots, bucket boundaries in the middle of a chunk), S in {1, 2, 4, 8} buckets per lane of k_pip_tiles, coarse bins of
2^5, 2^6 and 2^8 buckets, 1, 2, 4 and 8 lanes per bucket in k_pip_fold, rows of `sorted` padded by 0..3 entries, one
point past a block of the sort, both sides of the size at which the host-pointer MulVec changes its kernel, and the
extreme digits of every window.  The suite's other MulVec tests all have chunk length 8.

Every case asserts its regime from the shape msm_profile reports against tests/test_pip_shape_cpu.py REGIMES, which the
CPU suite pins to the host build of csrc/pip_shape.hpp (it adds S, fb, fl, cpw and the padding that the report lacks).

The expected value is the known-logarithm identity of test_gpu_msm.py finished on the CPU: points are drawn, with
repetition, from the 4096 points k g of PublicKey::new(2047) (k = 1, 2, 3 (i + 1), 5 (i + 1); publickey.rs:23-39),
so the result must be (sum_i s_i k_idx(i) mod r) g -- one scalar multiplication by the C oracle (pyref on edwards25519).
On the Weierstrass curves the pool is the oracle's own; on edwards25519 it is the engine's, with a sample checked
against pyref.  Every comparison is exact: wire words equal, status word 0."""

import random

import numpy as np
import pytest

import oracle as O
import pyref as P
from glv_cases import bls_split_scalars, secp_split_scalars
from gpu_util import msm_device_tensors, need_gpu
from test_gpu_msm import CURVES, msm_dev, to_words
from test_pip_shape_cpu import REGIMES

pytestmark = pytest.mark.gpu

POOL_LEN = 2047
INF = 2 * POOL_LEN + 2          # index of the point at infinity behind the pool (logarithm 0)
_POOLS = {}


class Pool:
    """per curve: the engine handle, the pool as wire points on the host and on the device, its logarithms"""

    def __init__(self, torch, B, cname, cid):
        self.cname, self.cid = cname, cid
        self.kind = "ed" if cid == 2 else "glv"
        self.r = P.CURVES[cname]["r"]
        self.a = B.Arith.init(cid)
        self.logs = np.array([1, 2] + [3 * (i + 1) for i in range(POOL_LEN)] + [5 * (i + 1) for i in range(POOL_LEN)] + [0],
                             dtype=np.int64)
        if cid == 2:
            self.G = P.EdwardsGroup(P.ED25519)
            pk = B.PublicKey.new(self.a, POOL_LEN)
            pts = np.concatenate([pk.gh, pk.G_vec, pk.H_vec])
            rnd = random.Random(5)
            sample = [0, 1, 2, 2 + POOL_LEN - 1, 2 + POOL_LEN, 2 * POOL_LEN + 1] + [rnd.randrange(pts.shape[0]) for _ in range(34)]
            for i in sample:
                assert O.wire_to_point(cid, pts[i]) == self.G.mul(self.G.base(), int(self.logs[i])), i
        else:
            pk = O.PublicKey(cid, POOL_LEN)
            pts = np.concatenate([pk.gh, pk.G, pk.H])
        self.pts = np.concatenate([pts, self.a.zero_point()[None]])
        assert self.pts.shape == (INF + 1, self.a.PW)
        self.d_pts = torch.from_numpy(self.pts.view(np.int64)).to("cuda:0")

    def expected(self, scalars, idx):
        """(sum_i s_i k_idx(i) mod r) g on the CPU.  scalars: (n, 4) u64.  Per pool index the 32-bit half-limbs of its
        scalars are summed by bincount -- in doubles, exactly: n 2^32 < 2^53 -- which leaves 8 x 4097 integer products."""
        n = scalars.shape[0]
        assert n < (1 << 21) and idx.shape == (n,)
        half = np.ascontiguousarray(scalars).view(np.uint32).reshape(n, 8)
        tot = 0
        for h in range(8):
            per = np.bincount(idx, weights=half[:, h].astype(np.float64), minlength=INF + 1)
            tot += sum(int(v) * int(k) for v, k in zip(per, self.logs) if v) << (32 * h)
        tot %= self.r
        if self.cid == 2:
            return O.point_to_wire(self.cid, self.G.mul(self.G.base(), tot) if tot else None)
        return O.point_mul(self.cid, O.generator(self.cid), tot)

    def check_shape(self, shape, n, c):
        row = REGIMES[(self.kind, n, c)]
        want = dict(n=n, items=2 * n if self.kind == "glv" else n, window_bits=row[0], windows=row[1], narrow_bits=row[2],
                    wide_windows=row[3], buckets=row[5], chunk_entries=row[7])
        assert shape == want, (self.cname, n, c)

    def run(self, torch, B, scalars, idx, c, exp=None):
        """the MulVec over pool[idx] through bpp_msm_device (points gathered on the device) == expected, in its regime"""
        d_sc = torch.from_numpy(np.ascontiguousarray(scalars).view(np.int64)).to("cuda:0")
        d_pt = self.d_pts[torch.from_numpy(idx).to("cuda:0")].contiguous()
        got, st, shape = msm_device_tensors(torch, B, self.a, d_sc, d_pt, c)
        self.check_shape(shape, scalars.shape[0], c)
        assert st == 0
        exp = self.expected(scalars, idx) if exp is None else exp
        assert np.array_equal(got, exp), (self.cname, scalars.shape[0], c)
        return exp


def pool(cname, cid):
    torch = need_gpu()
    import bulletproofsplus_amd as B
    if cid not in _POOLS:
        _POOLS[cid] = Pool(torch, B, cname, cid)
    return torch, B, _POOLS[cid]


def uniform_scalars(rng, n, r):
    """full-width values below 2^252 (below every curve's group order); 0, 1, r - 1 and a value >= r in the first slots"""
    sc = rng.randint(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    sc[:, 7] >>= 4
    sc = sc.view(np.uint64).reshape(n, 4)
    edge = to_words([0, 1, r - 1, r + 12345])
    sc[:min(n, 4)] = edge[:min(n, 4)]
    return sc


def test_expected_value_helper_matches_big_integers():
    """the bincount form of sum_i s_i k_idx(i) against the plain sum (no GPU work beyond the pool's set-up)"""
    _, _, pl = pool("secp256k1", 1)
    rng = np.random.RandomState(3)
    sc = uniform_scalars(rng, 3000, pl.r)
    idx = rng.randint(0, INF + 1, size=3000)
    tot = sum(int(s) * int(pl.logs[i]) for s, i in zip(O.wire_to_scalars(sc), idx)) % pl.r
    assert np.array_equal(pl.expected(sc, idx), O.point_mul(1, O.generator(1), tot))
    assert np.array_equal(pl.expected(sc[:300], idx[:300]), O.msm(1, sc[:300], pl.pts[idx[:300]]))


# ---- one case per regime, at the smallest n that reaches it ------------------------------------------------------
GLV_CASES = [((1 << 15) + 1, 2), ((1 << 16) + 1, 2), ((1 << 17) + 1, 2), (1 << 18, 12), (1 << 18, 15), (1 << 19, 13)]
ED_CASES = [(33027, 2), (66053, 2), (132105, 2), (1 << 18, 12), (1 << 18, 15), (1 << 19, 13)]
REGIME_CASES = [(cn, ci, n, c) for cn, ci in CURVES for n, c in (ED_CASES if ci == 2 else GLV_CASES)]


@pytest.mark.parametrize("cname,cid,n,c", REGIME_CASES)
def test_msm_regime(cname, cid, n, c):
    """chunk lengths 16 / 32 / 64 at width 2 (every bucket spread over hundreds of chunks: k_pip_fold_heavy, the Horner
    branch of k_pip_final, `sorted` rows padded by 1..3 entries) and at widths 12 / 13 / 15 (dense buckets folded by
    8 / 4 / 2 / 1 lanes, S = 2, coarse bins of 2^5, 2^6, 2^8 buckets)"""
    torch, B, pl = pool(cname, cid)
    rng = np.random.RandomState(n % 1000 + 17 * c + cid)
    pl.run(torch, B, uniform_scalars(rng, n, pl.r), rng.randint(0, INF, size=n), c)


@pytest.mark.parametrize("cname,cid", CURVES)
def test_msm_benchmark_regime_chunks_of_64(cname, cid):
    """n = 2^20 + 1, the smallest size with the benchmark's shape: width 16, chunk length 64, S = 8 on the GLV curves; on
    edwards25519 the chosen width is 15 (S = 2) and S = 4 is the explicit width 16.  Also with all scalars equal (one
    bucket per window holds every point: the heavy fold at chunk length 64) and with a quarter of the points at infinity."""
    torch, B, pl = pool(cname, cid)
    n = (1 << 20) + 1
    rng = np.random.RandomState(77 + cid)
    sc = uniform_scalars(rng, n, pl.r)
    idx = rng.randint(0, INF, size=n)
    exp = pl.run(torch, B, sc, idx, 0)
    if cid == 2:
        pl.run(torch, B, sc, idx, 16, exp)
    s1 = np.broadcast_to(sc[7], (n, 4)).copy()
    pl.run(torch, B, s1, idx, 0)
    idx[1::4] = INF
    pl.run(torch, B, sc, idx, 0)


# ---- block and padding boundaries ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2047, 2048, 2049, 4095, 4096, 4097, 8191])
@pytest.mark.parametrize("cname,cid", CURVES)
def test_msm_block_and_padding_boundaries(cname, cid, n):
    """sizes around a block of the sort (2048 points) and around the size from which the host-pointer MulVec takes this
    pipeline (4096), odd item counts; the device entry point and the host-pointer one must both give the CPU's value"""
    torch, B, pl = pool(cname, cid)
    rng = np.random.RandomState(n + cid)
    sc = uniform_scalars(rng, n, pl.r)
    idx = rng.randint(0, INF, size=n)
    exp = pl.run(torch, B, sc, idx, 0)
    pts = pl.pts[idx]
    got, st = msm_dev(torch, B, pl.a, sc, pts, 0, want_status=True)       # the same through host arrays
    assert st == 0 and np.array_equal(got, exp)
    assert np.array_equal(B.msm_batch(pl.a, sc, pts, [n])[0], exp)
    if n == 4097:
        for c in (2, 7, 16):
            pl.run(torch, B, sc, idx, c, exp)          # asserts the regime bpp_msm_pippenger then runs in
            assert np.array_equal(B.msm_pippenger(pl.a, sc, pts, c), exp), c


# ---- edge scalars ------------------------------------------------------------------------------------------------
def edge_scalars(cname):
    if cname == "bls12_381":
        return bls_split_scalars()
    if cname == "secp256k1":
        return secp_split_scalars()
    r = P.ED25519["r"]
    return [v for k in range(253) for v in (1 << k, (1 << k) - 1, r - (1 << k), r - (1 << k) + 1)]


@pytest.mark.parametrize("cname,cid", CURVES)
def test_msm_edge_scalars_every_window_extreme(cname, cid):
    """the edge lists of the scalar splits (edwards25519: 2^k, 2^k - 1, r - 2^k, r - 2^k + 1) through the whole pipeline:
    the extreme digits of every window and of the unsigned top window, at the last bucket of a window"""
    torch, B, pl = pool(cname, cid)
    ks = edge_scalars(cname)
    n = len(ks)
    sc = to_words(ks)
    idx = np.random.RandomState(8 + cid).randint(0, INF, size=n)
    exp = pl.expected(sc, idx)
    tot = sum(k * int(pl.logs[i]) for k, i in zip(ks, idx)) % pl.r
    assert np.array_equal(exp, pl.expected(to_words([tot]), np.zeros(1, dtype=np.int64)))   # logarithm 1: tot g
    for c in (0, 2, 5, 13, 16):
        pl.run(torch, B, sc, idx, c, exp)
