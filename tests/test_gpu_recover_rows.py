"""-m gpu: k_recover_masks (csrc/recover.hpp) on the synthetic rows of tests/recover_rows.py, through the public wire call
bpp_range_recover_masks_mixed_device with d_challenges and d_blinding (or a key) chosen by the test.

What only the device has -- the 16-lane group per proof, the butterflies of `sum` and `bad`, the idle groups of a short
last wave, the packed offsets RX_CH / RX_BLIND -- runs here at every k from 0 to 12 and with ZERO challenges, which no
transcript can draw: a zero row must come back as Gamma = 0 and leave the other proofs of its wave alone.  The expected Gamma
of a row is gamma_of(gammas, z) of a delta' built forward (recover_rows.make_row); every Gamma is compared bit for bit, and
d_out_masks sits between guards (test_gpu_recover._recover_device).

Verifiers are made with window_bits 3: the recovery reads no table.  The (1,64) verifier (k = 0..6 through its views) and
the (64,64) verifier (k = 6..12) are made on all three curves: a (64,64) build costs a fraction of a second (the figures
below include it).

Wall time per function on one MI355X, call phase, in one run with tests/test_gpu_verifier_scalars.py (slowest function there:
test_lds_opt_in_grows_and_the_smaller_shape_still_runs, 0.47 s, after 1.58 s of setup before the module's first test):
    test_every_k_and_every_row_in_one_mixed_call  (1,64): bls12_381 0.25 s (1.81 s of setup before it, the module's first
                                                  test), secp256k1 0.05 s, ed25519 0.05 s; (64,64), the verifier's build
                                                  included: bls12_381 0.13 s, secp256k1 0.13 s, ed25519 0.30 s
    test_a_zero_row_and_its_neighbours_in_a_wave  0.08 s
    test_every_zero_position_at_k_0_3_6_12        bls12_381 0.08 s, secp256k1 0.08 s, ed25519 0.07 s
    test_the_key_path                             bls12_381 0.10 s, secp256k1 0.09 s, ed25519 0.09 s
    test_the_host_twin                            0.08 s"""

import random

import pytest

import oracle as O
import recover_rows as RR
from gpu_util import need_gpu
from test_gpu_recover import _dev, _recover_device

pytestmark = pytest.mark.gpu

WINDOW_BITS = 3
MS = (1, 2, 4, 8, 16, 32, 64)
CROSS_COUNTS = (1, 2, 3, 4, 5, 7, 67)


@pytest.fixture(scope="module")
def engines():
    """verifiers by (curve, n, m), built on first use and closed with the module"""
    need_gpu()
    import bulletproofsplus_amd as B
    made, ariths = {}, {}

    def get(cname, n, m):
        if (cname, n, m) not in made:
            a = ariths.setdefault(cname, B.Arith.init(cname))
            made[(cname, n, m)] = B.BatchVerifier(B.PublicKey.new(a, n * m), n, m, window_bits=WINDOW_BITS)
        return made[(cname, n, m)]

    yield get
    for bv in made.values():
        bv.close()


def _call(torch, bv, rows, **kw):
    """one wire call over `rows` in this order: the packed challenge blocks, and the packed blinding unless kw names a key"""
    d_ch = _dev(torch, O.scalars_to_wire([x for row in rows for x in row.ch]))
    if "blind_key" not in kw:
        kw["blinding"] = [row.blind for row in rows]
    return _recover_device(torch, bv, [row.m for row in rows], [row.triple for row in rows], d_ch, **kw)


def _assert_rows(got, rows, what):
    wrong = [(i, row) for i, (g, row) in enumerate(zip(got, rows)) if g != row.gamma]
    assert len(got) == len(rows) and not wrong, "%s: %d of %d proofs differ, first %r" % (what, len(wrong), len(rows), wrong[:6])


def _mixed_rows(cname, n, source, index_of=lambda i: 0):
    return [RR.make_row(cname, n, m, name, source, index_of(i)) for i, (m, name) in enumerate(RR.mixed_items(n, MS, source))]


@pytest.mark.parametrize("cname,n", [(c, n) for n in (1, 64) for c in RR.CURVES])
def test_every_k_and_every_row_in_one_mixed_call(engines, cname, n):
    """(1,64): k = 0..6, (64,64): k = 6..12.  m_of cycles through 1, 2, 4, .., 64, so all seven classes are in the call and
    RX_CH / RX_BLIND advance by a different amount per proof; every named row of every class, the zero rows at every
    position among them"""
    torch = need_gpu()
    rows = _mixed_rows(cname, n, "buffer")
    assert {row.k for row in rows} == set(range(7) if n == 1 else range(6, 13))
    assert [row.m for row in rows[:7]] == list(MS)
    for m in MS:
        assert [row.name for row in rows if row.m == m] == RR.row_names(RR.log2(n * m), "buffer")
    _assert_rows(_call(torch, engines(cname, n, 64), rows), rows, "%s (%d,64)" % (cname, n))


def _cross_pools(count_max):
    zero_names = [x for x in RR.row_names(3, "buffer") if RR.is_zero_name(x) and x != "zero(z)"]
    good_names = [x for x in RR.row_names(3, "buffer") if not RR.is_zero_name(x) or x == "zero(z)"]
    zeros = [RR.make_row("secp256k1", 8, 1, zero_names[i % len(zero_names)], "buffer", i) for i in range(count_max)]
    goods = [RR.make_row("secp256k1", 8, 1, good_names[i % len(good_names)], "buffer", i) for i in range(count_max)]
    assert all(row.bad and row.gamma == 0 for row in zeros) and not any(row.bad for row in goods)
    assert sum(1 for row in goods if row.gamma != 0) >= count_max - 8   # gamma_zero rows apart
    return zeros, goods


def cross_places(count):
    """where the odd row goes: first, last, each of the four group places of the first wave and of the last"""
    last_wave = (count - 1) // 4 * 4
    return sorted({p for p in list(range(4)) + list(range(last_wave, last_wave + 4)) + [count - 1] if p < count})


def test_a_zero_row_and_its_neighbours_in_a_wave(engines):
    """one-class verifier (8,1), four proofs per wave.  One zero row at each group place of the first and of the last wave,
    first and last included -- last in a short wave, the idle groups repeat the BAD proof -- and every neighbour exact; then
    the mirror, every row a zero row but one: a lost flag shows as a non-zero mask, a leaked one as a zeroed neighbour"""
    torch = need_gpu()
    bv = engines("secp256k1", 8, 1)
    zeros, goods = _cross_pools(max(CROSS_COUNTS))
    for count in CROSS_COUNTS:
        places = cross_places(count)
        assert 0 in places and count - 1 in places
        for p in places:
            rows = [zeros[i] if i == p else goods[i] for i in range(count)]
            _assert_rows(_call(torch, bv, rows), rows, "count %d, zero row at %d" % (count, p))
            rows = [goods[i] if i == p else zeros[i] for i in range(count)]
            _assert_rows(_call(torch, bv, rows), rows, "count %d, the one good row at %d" % (count, p))


@pytest.mark.parametrize("cname", RR.CURVES)
def test_every_zero_position_at_k_0_3_6_12(engines, cname):
    """zero(y), zero(z) -- defined at m = 1, zero at m = 2 --, zero(e) and each zero(e_t), with one random row between two
    zero rows, at k = 0 (1,1), 1 (1,2), 3 (1,8) and (8,1), 6 (1,64) and (64,1), 7 (64,2) and 12 (64,64)"""
    torch = need_gpu()
    for n, cap, ms in ((1, 64, (1, 2, 8, 64)), (64, 64, (1, 2, 64)), (8, 1, (1,))):
        rows = []
        for m in ms:
            names = [x for x in RR.row_names(RR.log2(n * m), "buffer") if RR.is_zero_name(x)]
            assert len(names) == 3 + RR.log2(n * m)
            for i, name in enumerate(names):
                rows += [RR.make_row(cname, n, m, name, "buffer", i), RR.make_row(cname, n, m, "random", "buffer", i)]
        defined = [row for row in rows if row.name == "zero(z)" and row.m == 1]
        assert len(defined) == (1 if 1 in ms else 0) and all(not row.bad and row.gamma == row.gammas[0] for row in defined)
        assert all(row.bad for row in rows if RR.is_zero_name(row.name) and row not in defined)
        _assert_rows(_call(torch, engines(cname, n, cap), rows), rows, "%s (%d,%d)" % (cname, n, cap))


@pytest.mark.parametrize("cname", RR.CURVES)
def test_the_key_path(engines, cname):
    """the same rows with the blinding expanded from (key, index) by hashlib: index_base + position across 2^32, then
    d_index as a shuffled list.  edwards25519 has no prover in this suite; the synthetic rows need none."""
    torch = need_gpu()
    bv = engines(cname, 1, 64)
    base = (1 << 32) - 40
    rows = _mixed_rows(cname, 1, "key", lambda i: base + i)
    assert rows[0].index < 1 << 32 <= rows[-1].index
    _assert_rows(_call(torch, bv, rows, blind_key=RR.OWNER, index_base=base), rows, cname + " index_base")
    index = [base + i for i in range(len(rows))] + [(1 << 64) - 1, 0, 1 << 63]
    random.Random(5).shuffle(index)
    rows = _mixed_rows(cname, 1, "key", lambda i: index[i])
    _assert_rows(_call(torch, bv, rows, blind_key=RR.OWNER, index=index[:len(rows)]), rows, cname + " d_index")
    # another key reads other numbers out of every row whose Gamma is defined
    got = _call(torch, bv, rows, blind_key=RR.FOREIGN[0], index=index[:len(rows)])
    assert all((g == 0) if row.bad else (g == RR.foreign_gamma(row, RR.FOREIGN[0], row.index) != row.gamma)
               for g, row in zip(got, rows))


def test_the_host_twin(engines):
    """bpp_range_recover_masks_mixed on one mixed call: host buffers in, the same Gammas out"""
    need_gpu()
    bv = engines("secp256k1", 1, 64)
    rows = _mixed_rows("secp256k1", 1, "buffer")
    sc = O.scalars_to_wire([x for row in rows for x in row.triple]).reshape(-1, 3, 4)
    got = bv.recover_masks(sc, [row.m for row in rows], [O.scalars_to_wire(row.ch) for row in rows],
                           blinding=[row.blind for row in rows])
    _assert_rows(got, rows, "host twin")
    base = (1 << 32) - 3
    rows = _mixed_rows("secp256k1", 1, "key", lambda i: base + i)
    sc = O.scalars_to_wire([x for row in rows for x in row.triple]).reshape(-1, 3, 4)
    got = bv.recover_masks(sc, [row.m for row in rows], [O.scalars_to_wire(row.ch) for row in rows], blind_key=RR.OWNER,
                           index_base=base)
    _assert_rows(got, rows, "host twin, key")
