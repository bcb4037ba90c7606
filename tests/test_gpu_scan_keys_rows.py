"""-m gpu: the many-key scan's two kernels -- k_recover_coeffs and k_scan_keys with pair_key_index / pair_gamma
(csrc/recover_keys.hpp), the bodies the find kernels share -- on the synthetic rows of tests/recover_rows.py, through
bpp_debug_scan_keys (csrc/tu_debug.hip: RecoverKeysImpl's own call_job, bind_class, launch_coeffs and launch_scan_keys on
host buffers; RecoverKeysImpl::scan derives its challenges itself and has no door for chosen ones).

Bit for bit, no tolerance:
  - each of the 2k + 4 coefficients [A0, c_alpha, c_delta, c_eta, c_dL.., c_dR..] of every row without a zero challenge
    against the closed forms in big integers (recover_rows.coeff_closed_forms), at every k from 0 to 12;
  - out_bad = 1 exactly on the zero rows (gamma_zero rows: 0 -- out_bad is what tells a Gamma that IS zero from one that is
    undefined: k_scan_keys writes BPP_SCAN_UNCONFIRMED and zero for the latter, BPP_SCAN_UNCONFIRMED and Gamma else);
  - out_masks[key][caller]: the row's chosen Gamma for the owning key, A0 + sum c_s slot_s with hashlib slots for the foreign
    keys -- at k = 11 and 12 the stride loop of pair_gamma runs a FOURTH time (25 and 27 live slots), at k = 0 five lanes of
    a group idle;
  - status 2 and zero under every key where status_in != 0, whatever the row; the neighbours in the wave exact; the places no
    launch position names keep their guards.
The (1,64) and the (64,64) verifier are made on all three curves, as in tests/test_gpu_recover_rows.py.

Wall time per function on one MI355X, call phase, in one run with tests/test_gpu_verifier_scalars.py (slowest function there
0.47 s); the (64,64) rows include the verifier's build:
    test_every_row_at_every_k                     (1,64): bls12_381 0.13 s, secp256k1 0.14 s, ed25519 0.12 s;
                                                  (64,64): bls12_381 0.25 s, secp256k1 0.26 s, ed25519 0.40 s
    test_the_fourth_stride_under_nine_keys        bls12_381 0.14 s, secp256k1 0.15 s, ed25519 0.11 s
    test_counts_on_one_small_shape                count 1: 0.01 s, 5: 0.01 s, 67: 0.10 s
    test_a_zero_row_and_its_neighbours_in_a_wave  0.72 s (70 calls of the hook)
    test_a_rejected_place_and_its_neighbours      0.03 s
    test_errors_write_nothing                     below 0.005 s"""

import ctypes
import random

import numpy as np
import pytest

import oracle as O
import recover_cases as RC
import recover_rows as RR
from gpu_util import need_gpu
from test_gpu_recover_rows import CROSS_COUNTS, MS, cross_places, engines  # noqa: F401  (engines: the module's fixture)

pytestmark = pytest.mark.gpu

GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)
GUARD32 = np.uint32(0xA5A5A5A5)
UNCONFIRMED, FORMAT_ERROR, E_ARG = 3, 2, -1
KEYS = [RR.OWNER] + RR.FOREIGN   # nine


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Call:
    """the buffers of one call of the hook, guards in every output"""

    def __init__(self, rows, keys, total=None, caller=None, status_in=None, index=None, index_base=0):
        count, k = len(rows), rows[0].k
        self.count, self.k, self.keys = count, k, keys
        self.total = count if total is None else total
        self.s3 = O.scalars_to_wire([x for row in rows for x in row.triple]).reshape(count, 3, 4)
        self.ch = O.scalars_to_wire([x for row in rows for x in row.ch]).reshape(count, 3 + k, 4)
        self.status_in = None if status_in is None else np.asarray(status_in, dtype=np.uint32)
        self.caller = None if caller is None else np.asarray(caller, dtype=np.uint32)
        self.kb = np.frombuffer(b"".join(keys), dtype=np.uint8).copy() if keys else None
        self.index = None if index is None else np.asarray(index, dtype=np.uint64)
        self.index_base = index_base
        self.coeffs = np.full((count, 2 * k + 4, 4), GUARD, dtype=np.uint64)
        self.bad = np.full((count,), GUARD32, dtype=np.uint32)
        self.masks = np.full((len(keys), self.total, 4), GUARD, dtype=np.uint64)
        self.status = np.full((len(keys), self.total), GUARD32, dtype=np.uint32)

    def run(self, bv, m_view, **null):
        """the hook's return code; null: names of arguments to pass as NULL"""
        from bulletproofsplus_amd import _lib
        arg = lambda name: None if name in null else _ptr(getattr(self, name))
        return _lib.lib().bpp_debug_scan_keys(
            None if "v" in null else bv.handle, m_view, arg("s3"), arg("ch"), arg("status_in"), arg("caller"), self.count,
            self.total, arg("kb"), len(self.keys), ctypes.c_uint64(self.index_base), arg("index"), arg("coeffs"), arg("bad"),
            arg("masks") if self.keys else None, arg("status") if self.keys else None)

    def untouched(self):
        return bool((self.coeffs == GUARD).all() and (self.bad == GUARD32).all() and (self.masks == GUARD).all() and
                    (self.status == GUARD32).all())


def _ints(a):
    return [int(x) for x in O.wire_to_scalars(a)]


def _check(bv, m_view, rows, keys, what, total=None, caller=None, status_in=None, index=None, index_base=0):
    """one call, and everything it wrote against the rows.  A row's index must be the blinding index of its caller position."""
    from bulletproofsplus_amd import _lib
    r = RC.ORDER[rows[0].cname]
    c = Call(rows, keys, total, caller, status_in, index, index_base)
    _lib.check(c.run(bv, m_view), "bpp_debug_scan_keys")
    at = list(range(c.count)) if caller is None else list(caller)
    for i, row in enumerate(rows):
        assert row.index == (index[at[i]] if index is not None else index_base + at[i]), "the test's own bookkeeping"
    assert c.bad.tolist() == [1 if row.bad else 0 for row in rows], "%s: out_bad %s" % (what, c.bad.tolist())
    for i, row in enumerate(rows):
        if not row.bad:
            want = RR.coeff_closed_forms(r, row.n, row.m, row.triple[2], row.ch)
            got = _ints(c.coeffs[i])
            assert got == want, "%s: proof %d %r: coefficients %s differ" % (
                what, i, row, [s for s in range(len(want)) if got[s] != want[s]])
    for key_no, key in enumerate(keys):
        for i, row in enumerate(rows):
            rejected = status_in is not None and status_in[i] != 0
            if rejected or row.bad:
                want = 0
            else:
                want = row.gamma if key == RR.OWNER else RR.foreign_gamma(row, key, row.index)
            got = _ints(c.masks[key_no, at[i]])[0]
            assert got == want, "%s: key %d, proof %d at %d, %r: Gamma %x, expected %x" % (what, key_no, i, at[i], row, got, want)
            assert c.status[key_no, at[i]] == (FORMAT_ERROR if rejected else UNCONFIRMED), (what, key_no, i, row)
        for place in set(range(c.total)) - set(at):
            assert (c.masks[key_no, place] == GUARD).all() and c.status[key_no, place] == GUARD32, (what, key_no, place)
    return c


def _indices(total, seed):
    """total distinct blinding indices, some on either side of 2^32 and the ends of u64 among them"""
    rng = random.Random(seed)
    out = [(1 << 32) - 2 + i for i in range(total - 3)] + [0, (1 << 64) - 1, 1 << 63]
    rng.shuffle(out)
    return out


def _class_rows(cname, n, m, names, index, caller):
    return [RR.make_row(cname, n, m, name, "key", index[caller[i]]) for i, name in enumerate(names)]


@pytest.mark.parametrize("cname,n", [(c, n) for n in (1, 64) for c in RR.CURVES])
def test_every_row_at_every_k(engines, cname, n):
    """the views of (1,64): k = 0..6; of (64,64): k = 6..12, the fourth stride at 11 and 12.  Every named row of the class
    in one call, under 1, 3 or 9 keys, count x n_keys no multiple of 8 (a short last wave of k_scan_keys), a shuffled
    `caller` into total = count + 3 places and the index as a list"""
    need_gpu()
    bv = engines(cname, n, 64)
    seen = set()
    for j, m in enumerate(MS):
        k = RR.log2(n * m)
        n_keys = (1, 3, 9)[(j + (0 if n == 1 else 1)) % 3]
        names = RR.row_names(k, "key")
        if len(names) * n_keys % 8 == 0:
            names = names + ["random"]
        count = len(names)
        assert count * n_keys % 8 and {"zero(e_%d)" % t for t in range(k)} <= set(names)
        caller = random.Random(100 + k).sample(range(count + 3), count)
        index = _indices(count + 3, k)
        rows = _class_rows(cname, n, m, names, index, caller)
        _check(bv, 0 if m == 64 else m, rows, KEYS[:n_keys], "%s (%d,%d) %d keys" % (cname, n, m, n_keys), total=count + 3,
               caller=caller, index=index)
        seen.add((k, n_keys))
    if n == 64:
        assert {(10, 9), (11, 1), (12, 3)} <= seen
    else:
        assert {(0, 1), (3, 1), (6, 1)} <= seen


@pytest.mark.parametrize("cname", RR.CURVES)
def test_the_fourth_stride_under_nine_keys(engines, cname):
    """k = 11 and 12 once more with nine keys each and k = 0 with three and nine: 25 and 27 live slots, and 3 (five idle
    lanes of the group), under every key count of the issue"""
    need_gpu()
    for n, m, n_keys in ((64, 32, 9), (64, 32, 3), (64, 64, 9), (64, 64, 1), (1, 1, 3), (1, 1, 9)):
        k = RR.log2(n * m)
        names = ["random", "one", "zero(e)", "minus_one", "top(0)", "gamma_zero", "delta_edges(0)"]
        caller = random.Random(200 + k).sample(range(10), 7)
        index = _indices(10, 50 + k)
        rows = _class_rows(cname, n, m, names, index, caller)
        _check(engines(cname, n, 64), 0 if m == 64 else m, rows, KEYS[:n_keys], "%s (%d,%d) %d keys" % (cname, n, m, n_keys),
               total=10, caller=caller, index=index)


def _pools(count_max, base):
    zero_names = [x for x in RR.row_names(3, "key") if RR.is_zero_name(x) and x != "zero(z)"]
    good_names = [x for x in RR.row_names(3, "key") if not RR.is_zero_name(x) or x == "zero(z)"]
    zeros = [RR.make_row("secp256k1", 8, 1, zero_names[i % len(zero_names)], "key", base + i) for i in range(count_max)]
    goods = [RR.make_row("secp256k1", 8, 1, good_names[i % len(good_names)], "key", base + i) for i in range(count_max)]
    assert all(row.bad for row in zeros) and not any(row.bad for row in goods)
    return zeros, goods


@pytest.mark.parametrize("count", [1, 5, 67])
def test_counts_on_one_small_shape(engines, count):
    """(8,1) secp256k1, the verifier's own shape: 1, 5 and 67 proofs -- a lone group, a second wave of k_recover_coeffs with
    one proof and three idle groups, seventeen waves -- under three keys (3, 15, 201 pairs: a short last wave each), no
    `caller`, no index list: index_base + position across 2^32"""
    need_gpu()
    base = (1 << 32) - 3
    zeros, goods = _pools(count, base)
    rows = [zeros[i] if i % 5 == 3 else goods[i] for i in range(count)]
    _check(engines("secp256k1", 8, 1), 0, rows, KEYS[:3], "count %d" % count, index_base=base)
    c = Call(rows, [])   # n_keys = 0: the coefficients alone
    from bulletproofsplus_amd import _lib
    _lib.check(c.run(engines("secp256k1", 8, 1), 0), "bpp_debug_scan_keys")
    assert c.bad.tolist() == [1 if row.bad else 0 for row in rows] and not (c.coeffs == GUARD).all(axis=2).any()


def test_a_zero_row_and_its_neighbours_in_a_wave(engines):
    """k_recover_coeffs has four proofs per wave: one zero row at each group place of the first and of the last wave, first
    and last included (last in a short wave: the idle groups repeat the BAD proof), then the mirror, all zero rows but one.
    out_bad exact, every neighbour's coefficients and Gammas exact, the zero row zero under all three keys"""
    need_gpu()
    bv = engines("secp256k1", 8, 1)
    base = 1 << 40
    zeros, goods = _pools(max(CROSS_COUNTS), base)
    for count in CROSS_COUNTS:
        for p in cross_places(count):
            rows = [zeros[i] if i == p else goods[i] for i in range(count)]
            _check(bv, 0, rows, KEYS[:3], "count %d, zero row at %d" % (count, p), index_base=base)
            rows = [goods[i] if i == p else zeros[i] for i in range(count)]
            _check(bv, 0, rows, KEYS[:3], "count %d, the one good row at %d" % (count, p), index_base=base)


def test_a_rejected_place_and_its_neighbours(engines):
    """status_in != 0 on a good row and on a zero row: 2 and zero under every key; the pairs beside them in the wave of
    k_scan_keys (eight pairs per wave, proof-major) exact; unnamed places keep their guards"""
    need_gpu()
    bv = engines("secp256k1", 8, 1)
    names = ["random", "one", "zero(y)", "top(0)", "zero(e_1)", "gamma_zero", "minus_one"]
    for rejected in ((1,), (2,), (0, 4), (1, 2, 6), tuple(range(7))):
        status_in = [0xdead if i in rejected else 0 for i in range(7)]
        caller = random.Random(len(rejected)).sample(range(10), 7)
        index = _indices(10, 7)
        rows = _class_rows("secp256k1", 8, 1, names, index, caller)
        c = _check(bv, 0, rows, KEYS[:3], "rejected %s" % (rejected,), total=10, caller=caller, status_in=status_in, index=index)
        assert c.bad.tolist() == [0, 0, 1, 0, 1, 0, 0]   # the flag is the challenge's, whatever the decoder said


def test_errors_write_nothing(engines):
    need_gpu()
    bv = engines("secp256k1", 1, 64)
    rows = [RR.make_row("secp256k1", 1, 4, "random", "key", i) for i in range(3)]
    for null in ("v", "s3", "ch", "coeffs", "bad", "kb", "masks", "status"):
        c = Call(rows, KEYS[:2])
        assert c.run(bv, 4, **{null: True}) == E_ARG and c.untouched(), null
    for m_view in (3, 64, 128, 6):   # neither 0 nor a power of two below m = 64
        c = Call(rows, KEYS[:2])
        assert c.run(bv, m_view) == E_ARG and c.untouched(), m_view
    c = Call(rows, KEYS[:2], total=2)
    c.masks = np.full((2, 3, 4), GUARD, dtype=np.uint64)   # what the hook must not reach
    c.status = np.full((2, 3), GUARD32, dtype=np.uint32)
    assert c.run(bv, 4) == E_ARG and c.untouched()   # total < count
    c = Call(rows, KEYS[:2], caller=[0, 3, 1])
    assert c.run(bv, 4) == E_ARG and c.untouched()   # a caller position beyond total
    c = Call(rows, KEYS[:2])
    c.count = 0
    assert c.run(bv, 4) == 0 and c.untouched()       # count = 0: BPP_OK before any launch
    c = Call(rows, KEYS[:2])
    c.total = 0x7fffffff // 64                       # n_keys x total beyond one launch: refused before a buffer is read
    assert c.run(bv, 4) == E_ARG and c.untouched()
