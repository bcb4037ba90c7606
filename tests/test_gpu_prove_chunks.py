"""-m gpu: the fixed-stride provers across a chunk boundary of their workspace.

prove_chunk caps a chunk at 2 048 proofs, so 2 048 + 3 proofs of shape (8, 1) is the smallest call with a second chunk.  Its
records, triples, commitments and challenge blocks must be byte for byte those of two single-chunk calls -- 2 048 proofs at
index_base, then 3 proofs at index_base + 2 048 over the tail of the same inputs -- which is what pins the per-chunk offsets
of every input and output, the slice of d_blinding and the blinding index of blind_key.  Single-chunk calls are pinned to
the oracle by test_gpu_prover_rows.py and test_gpu_prove_mixed.py (range) and test_gpu_wip.py (the seam).  Every output goes
into a sentinel-filled buffer with a guard behind it: nothing outside the expected extent may change."""

import numpy as np
import pytest

from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

N, M, K = 8, 1, 3
CHUNK, TAIL = 2048, 3
COUNT = CHUNK + TAIL
INDEX_BASE = 5
KEY = bytes(range(1, 33))
SENT = 0x5A
GUARD = 256   # bytes behind every output
CURVES = ("bls12_381", "secp256k1")   # the 13-limb field and a 9-limb one


@pytest.fixture(scope="module")
def engines():
    """(arith, verifier) of shape (8, 1) by curve, built on first use and closed with the module"""
    need_gpu()
    import bulletproofsplus_amd as B
    made = {}

    def get(cname):
        if cname not in made:
            a = B.Arith.init(cname)
            made[cname] = (a, B.BatchVerifier(B.PublicKey.new(a, N * M), N, M, window_bits=6))
        return made[cname]

    yield get
    for _, bv in made.values():
        bv.close()


def _scalars(rng, *shape):
    """canonical non-zero scalars in wire form, below 2^252 and so below every curve's group order"""
    return rng.integers(1, 1 << 60, size=shape + (4,), dtype=np.uint64)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(torch.device("cuda:0"))


def _out(torch, nbytes):
    return torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device="cuda:0")


def _take(t, nbytes, what):
    """the first nbytes of an output buffer, its guard checked"""
    h = t.cpu().numpy()
    assert (h[nbytes:] == SENT).all(), "%s: written beyond %d bytes" % (what, nbytes)
    return h[:nbytes]


def _range(torch, a, bv, values, gammas, index_base, transcript, blind_key=None, blinding=None):
    """bpp_range_prove_batch_device / _fs_device -> [records, triples, commitments, challenges] as bytes"""
    count, pw = len(values), a.PW * 8
    sizes = [count * (3 + 2 * K) * pw, count * 96, count * M * pw, count * (3 + K) * 32]
    d_v, d_g = _dev(torch, values), _dev(torch, gammas)
    d_b = _dev(torch, blinding) if blinding is not None else None
    outs = [_out(torch, sz) for sz in sizes]
    wsb = bv.prover_workspace_bytes(count)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    bv.prove_batch_device(d_v.data_ptr(), d_g.data_ptr(), count, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                          d_ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream, transcript=transcript,
                          d_out_challenges=outs[3].data_ptr() if transcript else 0, blind_key=blind_key, index_base=index_base,
                          d_blinding=d_b.data_ptr() if d_b is not None else 0)
    torch.cuda.synchronize()
    if not transcript:   # the literal entry has no challenges to give
        sizes[3] = 0
    return [_take(t, sz, "output %d" % i) for i, (t, sz) in enumerate(zip(outs, sizes))]


def _assert_split(whole, head, tail, what):
    for i, (w, h, t) in enumerate(zip(whole, head, tail)):
        assert len(w) == len(h) + len(t)
        assert (w != SENT).any() or len(w) == 0, (what, i, "nothing written")
        assert np.array_equal(w[:len(h)], h), (what, i, "first chunk")
        assert np.array_equal(w[len(h):], t), (what, i, "second chunk")


def _range_inputs(seed):
    rng = np.random.default_rng(seed)
    values = rng.integers(0, 1 << N, size=(COUNT, M), dtype=np.uint64)
    return values, _scalars(rng, COUNT, M), _scalars(rng, COUNT, 5 + 2 * K)


@pytest.mark.parametrize("source", ["blind_key", "d_blinding"])
@pytest.mark.parametrize("cname", CURVES)
def test_transcript_prover_across_the_chunk_boundary(engines, cname, source):
    torch = need_gpu()
    a, bv = engines(cname)
    values, gammas, blinding = _range_inputs(1)
    key = KEY if source == "blind_key" else None

    def call(lo, hi):
        return _range(torch, a, bv, values[lo:hi], gammas[lo:hi], INDEX_BASE + lo, True, blind_key=key,
                      blinding=None if key else blinding[lo:hi])

    whole, head, tail = call(0, COUNT), call(0, CHUNK), call(CHUNK, COUNT)
    _assert_split(whole, head, tail, "%s, %s" % (cname, source))
    # the blinding index reaches the proofs: the tail at the head's indices is another block of proofs
    if key:
        moved = _range(torch, a, bv, values[CHUNK:], gammas[CHUNK:], INDEX_BASE, True, blind_key=key)
        assert not np.array_equal(moved[0], tail[0])


@pytest.mark.parametrize("cname", CURVES)
def test_literal_prover_across_the_chunk_boundary(engines, cname):
    torch = need_gpu()
    a, bv = engines(cname)
    values, gammas, _ = _range_inputs(2)
    whole, head, tail = (_range(torch, a, bv, values[lo:hi], gammas[lo:hi], 0, False)
                         for lo, hi in ((0, COUNT), (0, CHUNK), (CHUNK, COUNT)))
    _assert_split(whole, head, tail, "%s, literal" % cname)


def _seam(torch, a, bv, av, bvec, y, gamma, states, index_base, blind_key=None, blinding=None):
    """bpp_wip_prove_batch_device at nv = 0 under a transcript -> [records, triples, challenges] as bytes"""
    count, pw = len(av), a.PW * 8
    npts = bv.wip_points_per_proof(0)
    sizes = [count * npts * pw, count * 96, count * (1 + K) * 32]
    ins = [_dev(torch, x) for x in (av, bvec, y, gamma, states)]
    d_b = _dev(torch, blinding) if blinding is not None else None
    outs = [_out(torch, sz) for sz in sizes]
    wsb = bv.wip_prover_workspace_bytes(count)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    bv.wip_prove_device(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), count, 0, outs[0].data_ptr(),
                        outs[1].data_ptr(), d_ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream, transcript=True,
                        d_transcript=ins[4].data_ptr(), blind_key=blind_key, index_base=index_base,
                        d_blinding=d_b.data_ptr() if d_b is not None else 0, d_out_challenges=outs[2].data_ptr())
    torch.cuda.synchronize()
    got = [_take(t, sz, "output %d" % i) for i, (t, sz) in enumerate(zip(outs, sizes))]
    rec = got[0].reshape(count, npts, pw)
    assert (rec[:, 0] == SENT).all(), "point 0 of a record is the caller's"
    return got


@pytest.mark.parametrize("source", ["d_blinding", "blind_key"])
@pytest.mark.parametrize("cname", CURVES)
def test_seam_prover_across_the_chunk_boundary(engines, cname, source):
    torch = need_gpu()
    a, bv = engines(cname)
    rng = np.random.default_rng(3)
    length = N * M
    av, bvec = _scalars(rng, COUNT, length), _scalars(rng, COUNT, length)
    y, gamma, blinding = _scalars(rng, COUNT), _scalars(rng, COUNT), _scalars(rng, COUNT, 5 + 2 * K)
    states = rng.integers(0, 256, size=(COUNT, 32), dtype=np.uint8)
    key = KEY if source == "blind_key" else None

    def call(lo, hi):
        return _seam(torch, a, bv, av[lo:hi], bvec[lo:hi], y[lo:hi], gamma[lo:hi], states[lo:hi], INDEX_BASE + lo,
                     blind_key=key, blinding=None if key else blinding[lo:hi])

    whole, head, tail = call(0, COUNT), call(0, CHUNK), call(CHUNK, COUNT)
    _assert_split(whole, head, tail, "%s seam, %s" % (cname, source))
