"""-m gpu: the verifier's scalar stage -- k_vs_prepare / k_vs_expand (csrc/kernels.hpp) through launch_verify_scalars, and the
seam's k_wvs_prepare / k_wvs_expand (csrc/wip_seam.hpp) -- on CHOSEN challenges, at every shape at which the kernels take
another path.  The range path runs through bpp_debug_verifier_scalars (csrc/tu_debug.hip: the function every pass calls, on
host buffers), the seam through bpp_wip_verify_batch_device's d_challenges and d_out_scalars.

Expected values come from tests/scalar_cases.py alone (pyref's verify_mulvec for the rows pyref can take, the written-out
closed forms with inv0(0) = 0 for a challenge that is 0 mod r; tests/test_scalar_cases_cpu.py holds the two to each other
and to the C oracle).  EVERY scalar of EVERY proof is compared, bit for bit.  Verifiers are made with window_bits 3, the
smallest this suite uses on all three curves, so that their tables stay small."""

import ctypes
import functools

import numpy as np
import pytest

import scalar_cases as S
from gpu_util import need_gpu, run_verifier_device

pytestmark = pytest.mark.gpu

WINDOW_BITS = 3
GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)
SMALL_COUNT = 73      # k_vs_prepare blocks of 64 + 9 proofs; ten k_vs_expand blocks of VS_PB = 8, the last with ONE proof
LARGE_COUNT = 9       # at (32,64) and (64,64): two k_vs_expand blocks, the last with one proof


@pytest.fixture(scope="module")
def engines():
    """verifiers by (curve, n, m), built on first use and closed with the module"""
    need_gpu()
    import bulletproofsplus_amd as B
    made, ariths = {}, {}

    def get(cname, n, m):
        if (cname, n, m) not in made:
            a = ariths.setdefault(cname, B.Arith.init(cname))
            pk = B.PublicKey.new(a, n * m)
            made[(cname, n, m)] = (a, pk, B.BatchVerifier(pk, n, m, window_bits=WINDOW_BITS))
        return made[(cname, n, m)]

    yield get
    for _, _, bv in made.values():
        bv.close()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _hook_rc(bv, m_view, s3, ch, count, out):
    from bulletproofsplus_amd import _lib
    return _lib.lib().bpp_debug_verifier_scalars(bv.handle, m_view, _ptr(s3), _ptr(ch), count, _ptr(out))


def _hook(bv, m_view, s3, ch, N):
    """one call of the hook over s3 (count, 3, 4), ch (count, 3 + k, 4) or None -> (count, N, 4); count >= 1"""
    from bulletproofsplus_amd import _lib
    count = s3.shape[0]
    assert count >= 1 and s3.shape == (count, 3, 4) and (ch is None or ch.shape[0] == count)
    out = np.full((count, N, 4), GUARD, dtype=np.uint64)
    _lib.check(_hook_rc(bv, m_view, s3, ch, count, out), "bpp_debug_verifier_scalars")
    return out


def _want(curve, n, m, row):
    """the definition of one row: pyref where it can be asked, the closed forms (inv0) for a zero challenge"""
    f = S.range_scalars_direct if row.name.startswith("zero") else S.range_scalars
    return f(curve, n, m, *row.args())


def _wires(curve, n, m, rows):
    k = S.log2(n * m)
    s3 = S.to_wire([x for row in rows for x in row.s3]).reshape(len(rows), 3, 4)
    ch = S.to_wire([x for row in rows for x in row.challenges()]).reshape(len(rows), 3 + k, 4)
    want = S.to_wire([x for row in rows for x in _want(curve, n, m, row)]).reshape(len(rows), S.n_scalars(n, m), 4)
    return s3, ch, want


@functools.lru_cache(maxsize=None)
def _batch(curve, n, m, count, seed, names=None):
    """rows cycling through `names` (default: every non-zero row of the shape) with their wire forms and expected scalars;
    computed once, shared, never written to"""
    rows = S.rows(curve, n, m, count, seed, names)
    out = (rows,) + _wires(curve, n, m, rows)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _assert_same(got, want, rows, what):
    if np.array_equal(got, want):
        return
    bad = np.argwhere((got != want).any(axis=2))
    names = sorted({rows[i].name for i in set(bad[:, 0].tolist())})
    raise AssertionError("%s: %d scalars differ in %d of %d proofs, rows %s; first (proof, row, scalar) %s" % (
        what, len(bad), len(set(bad[:, 0].tolist())), len(rows), names, [(int(i), rows[i].name, int(t)) for i, t in bad[:8]]))


def _sweep(bv, curve, n, m_own, m_view, count, seed):
    """all non-zero rows of the shape (n, m_view or m_own), `count` proofs per call, as many calls as the rows need"""
    m = m_view or m_own
    k = S.log2(n * m)
    names = S.row_names(k)
    calls = -(-len(names) // count)
    rows, s3, ch, want = _batch(curve, n, m, calls * count, seed)
    assert {r.name for r in rows} == set(names) and {"one_hot(%d)" % t for t in range(k)} <= set(names)
    for c in range(calls):
        sl = slice(c * count, (c + 1) * count)
        got = _hook(bv, m_view, s3[sl], ch[sl], S.n_scalars(n, m))
        _assert_same(got, want[sl], rows[sl], "%s (%d,%d) view %d call %d" % (curve, n, m_own, m_view, c))


# ---- 1. the dynamic-LDS opt-in: a shape above 64 KB, then a larger one, then the smaller again ----------------------------
def test_lds_opt_in_grows_and_the_smaller_shape_still_runs(engines):
    """(32,64) asks for more dynamic LDS than the default limit, (64,64) for more again (CH = 32, then 64): the record of
    the largest opt-in so far must grow, and must not shrink the limit under the (64,64) launch that follows."""
    curve = "bls12_381"
    _, _, small = engines(curve, 32, 64)
    _sweep(small, curve, 32, 64, 0, LARGE_COUNT, 1)
    _, _, large = engines(curve, 64, 64)
    _sweep(large, curve, 64, 64, 0, LARGE_COUNT, 1)
    _sweep(small, curve, 32, 64, 0, LARGE_COUNT, 1)
    _sweep(large, curve, 64, 64, 0, LARGE_COUNT, 1)


@pytest.mark.parametrize("m_view", [1, 2, 4, 16, 32])
def test_views_of_the_largest_verifier(engines, m_view):
    """(64, m'): CH = m' indices per lane, next to the verifier's own CH = 64 above"""
    _, _, bv = engines("bls12_381", 64, 64)
    _sweep(bv, "bls12_381", 64, 64, m_view, LARGE_COUNT, 2)


# ---- 2. the small shapes, own shape and every view, 73 proofs a call ------------------------------------------------------
# (8,16): CH = 2, n < 64, mn 8..128.  (2,64): CH = n = 2, pz[] changes on every lane.  (1,64): n = 1 -- i0 % 1, sum_of_powers'
# n = 1 quirk -- and, as its view 1, the shape (1,1) with k = 0.  (1,1) as a verifier of its own: bpp_verifier_create takes it.
# (4,8): mn = 32 < 64, lanes 32..63 idle.
SMALL_SHAPES = [(8, 16, (1, 2, 4, 8)), (2, 64, (1, 2, 32)), (1, 64, (1, 2, 32)), (1, 1, ()), (4, 8, (1, 4))]


@pytest.mark.parametrize("n,m,views", SMALL_SHAPES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("curve", S.CURVES)
def test_shape_sweep(engines, curve, n, m, views):
    _, _, bv = engines(curve, n, m)
    for m_view in (0,) + views:
        _sweep(bv, curve, n, m, m_view, SMALL_COUNT, 3)


# ---- 3. counts at the block boundaries; count 0 ------------------------------------------------------------------------
@pytest.mark.parametrize("curve", S.CURVES)
def test_counts_around_a_block_of_expand(engines, curve):
    n, m = 8, 16
    _, _, bv = engines(curve, n, m)
    N = S.n_scalars(n, m)
    rows, s3, ch, want = _batch(curve, n, m, 25, 4)
    at = 0
    for count in (1, 7, 8, 9):
        sl = slice(at, at + count)
        _assert_same(_hook(bv, 0, s3[sl], ch[sl], N), want[sl], rows[sl], "%s count %d" % (curve, count))
        at += count
    # count 0: OK, and nothing is written
    out = np.full((2, N, 4), GUARD, dtype=np.uint64)
    assert _hook_rc(bv, 0, s3[:1].copy(), ch[:1].copy(), 0, out) == 0
    assert (out == GUARD).all()


def test_hook_refuses_bad_arguments(engines):
    from bulletproofsplus_amd import _lib
    n, m = 8, 16
    _, _, bv = engines("secp256k1", n, m)
    rows, s3, ch, want = _batch("secp256k1", n, m, 25, 4)
    s3, ch = s3[:2].copy(), ch[:2].copy()
    out = np.full((2, S.n_scalars(n, m), 4), GUARD, dtype=np.uint64)
    for m_view in (3, 16, 32):
        assert _hook_rc(bv, m_view, s3, ch, 2, out) == -1
        assert "m_view" in _lib.lib().bpp_last_error().decode()
    assert _hook_rc(bv, 0, None, ch, 2, out) == -1
    assert _hook_rc(bv, 0, s3, ch, 2, None) == -1
    assert (out == GUARD).all()


# ---- 4. a challenge that is 0 mod r -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,m_own", [(8, 2, 2), (64, 1, 1), (8, 16, 16)])
@pytest.mark.parametrize("curve", S.CURVES)
def test_zero_rows_alone_among_healthy_neighbours(engines, curve, n, m, m_own):
    """each zero row (y, e, the first and the last round challenge; as 0 and as words that are a multiple of r) in a batch
    of nine healthy rows, at a position that walks over both k_vs_expand blocks: its scalars are the closed forms' with
    inv0(0) = 0, and the neighbours' are bit-identical to those of the batch with a healthy row in its place"""
    _, _, bv = engines(curve, n, m_own)
    k, N = S.log2(n * m), S.n_scalars(n, m)
    names = S.zero_row_names(k)
    zrows = _batch(curve, n, m, len(names), 5, tuple(names))[0]
    healthy, hs3, hch, hwant = _batch(curve, n, m, LARGE_COUNT, 6, ("random", "lifted", "minus_ones"))
    base = _hook(bv, 0, hs3, hch, N)
    _assert_same(base, hwant, healthy, "%s (%d,%d) healthy batch" % (curve, n, m))
    r = S.order(curve)
    for j, zrow in enumerate(zrows):
        p = (0, 7, 8, 3)[j % 4]
        rows = list(healthy)
        rows[p] = zrow
        s3, ch, want = _wires(curve, n, m, rows)
        zv = [zrow.y, zrow.e] + zrow.e_rounds
        assert sum(1 for x in zv if x % r == 0) == 1 and ("lifted" in zrow.name) == any(x >= r and x % r == 0 for x in zv)
        got = _hook(bv, 0, s3, ch, N)
        assert np.array_equal(got[p], want[p]), (zrow.name, np.argwhere((got[p] != want[p]).any(axis=1))[:8].ravel().tolist())
        others = [i for i in range(LARGE_COUNT) if i != p]
        assert np.array_equal(got[others], base[others]), zrow.name


# ---- 5. the literals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,m_view", [(2, 64, 0), (8, 16, 0), (8, 16, 1)])
@pytest.mark.parametrize("curve", S.CURVES)
def test_null_challenges_are_the_literals_of_the_shape(engines, curve, n, m, m_view):
    """no golden file covers these shapes: [y, z, e, e_t] = [12, 23, 99, 7..], and [7, 7, 99, 7..] for the view m' = 1"""
    _, _, bv = engines(curve, n, m)
    mp = m_view or m
    k = S.log2(n * mp)
    rows = [row.replace(y=7 if mp == 1 else 12, z=7 if mp == 1 else 23, e=99, e_rounds=[7] * k)
            for row in S.rows(curve, n, mp, LARGE_COUNT, 7, ["random", "proof_scalars(0)", "lifted"])]
    s3, _, want = _wires(curve, n, mp, rows)
    for row, w in zip(rows, want):
        assert np.array_equal(S.to_wire(S.range_scalars_direct(curve, n, mp, *row.args())), w)
    _assert_same(_hook(bv, m_view, s3, None, S.n_scalars(n, mp)), want, rows, "%s (%d,%d) literals" % (curve, n, mp))


# ---- 6. the hook is the public path; a view is a verifier of its own ----------------------------------------------------------
@pytest.mark.parametrize("curve", S.CURVES)
def test_hook_equals_the_public_pass_and_a_view_a_dedicated_verifier(engines, curve):
    torch = need_gpu()
    n, m = 8, 2
    k, N = S.log2(n * m), S.n_scalars(n, m)
    a, pk, bv = engines(curve, n, m)
    names = tuple(S.row_names(k) + S.zero_row_names(k))
    rows, s3, ch, want = _batch(curve, n, m, len(names), 8, names)
    got = _hook(bv, 0, s3, ch, N)
    _assert_same(got, want, rows, "%s (8,2)" % curve)
    # bpp_verifier_run's d_out_scalars for the same inputs (the records: any valid wire points)
    rec = np.broadcast_to(pk.gh[0], (len(rows), 3 + 2 * k + m, a.PW)).copy()
    _, pub, _ = run_verifier_device(torch, bv, rec, np.array(s3), want_result=False, challenges=np.array(ch))
    assert pub.shape == got.shape and np.array_equal(pub, got)
    # the (8,16) verifier's view m' = 2
    _, _, wide = engines(curve, 8, 16)
    assert np.array_equal(_hook(wide, 2, s3, ch, N), got)


# ---- 7. the seam -----------------------------------------------------------------------------------------------------------
class _SeamCtx:
    """what test_gpu_wip's _verify_device reads of its Ctx; the key is made on the device (Ctx builds it on the CPU,
    which takes seconds at 512 generators on edwards25519)"""

    def __init__(self, a, bv, length):
        self.bv, self.length, self.k, self.PW = bv, length, S.log2(length), a.PW


def _seam_engine(engines, curve, length):
    return engines(curve, min(length, 64), max(1, length // 64))


def _seam_want(curve, length, row):
    zero = row.name.startswith("zero") or row.y % S.order(curve) == 0
    return (S.seam_scalars_direct if zero else S.seam_scalars)(curve, length, *row.args())


def _seam_run(torch, engines, curve, length, nv, rows):
    from test_gpu_wip import _verify_device
    a, pk, bv = _seam_engine(engines, curve, length)
    cx = _SeamCtx(a, bv, length)
    count = len(rows)
    rec = np.broadcast_to(pk.gh[0], (count, 3 + 2 * cx.k + nv, a.PW)).copy()
    sc = S.to_wire([x for row in rows for x in row.s3]).reshape(count, 3, 4)
    ch = S.to_wire([x for row in rows for x in row.challenges()]).reshape(count, 1 + cx.k, 4)
    return _verify_device(torch, cx, rec, sc, [row.y for row in rows], [row.stm for row in rows], nv, challenges=ch)


def _seam_check(curve, length, nv, rows, osc):
    N = 2 * length + 2 * S.log2(length) + 5 + nv
    want = S.to_wire([x for row in rows for x in _seam_want(curve, length, row)]).reshape(len(rows), N, 4)
    _assert_same(osc, want, rows, "seam %s length %d nv %d" % (curve, length, nv))


@pytest.mark.parametrize("nv", [0, 1, 3])
@pytest.mark.parametrize("length", [4, 64, 128, 512])
@pytest.mark.parametrize("curve", S.CURVES)
def test_seam_scalars_on_chosen_challenges(engines, curve, length, nv):
    """lengths with CH = 1 (4: idle lanes; 64), 2 and 8; 73 proofs; per-proof [e, e_1..e_k] cycling through random,
    one_hot(t) for every t, ones, minus ones, lifted (y too), y = 2^-1, e = 0 and a zero first / last round challenge"""
    torch = need_gpu()
    k = S.log2(length)
    rows = S.seam_rows(curve, length, nv, SMALL_COUNT, 9)
    assert {r.name for r in rows} == set(S.seam_row_names(k)) and len(S.seam_row_names(k)) == k + 8
    _, osc, _ = _seam_run(torch, engines, curve, length, nv, rows)
    _seam_check(curve, length, nv, rows, osc)


def test_seam_takes_every_nv_the_entry_point_allows(engines):
    """wvs_lds_bytes counts e_t^2, y^-(2^b), the two low-bit tables and a few constants: it depends on the LENGTH alone, and
    stays under the 64 KB the entry point allows at every length an engine can have (n, m <= 64).  What bounds nv is
    VS_MAXM = 64: nv = 64 runs, nv = 65 is BPP_E_ARG."""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    curve, length, nv = "secp256k1", 512, 64
    rows = S.seam_rows(curve, length, nv, SMALL_COUNT, 10)
    _, osc, _ = _seam_run(torch, engines, curve, length, nv, rows)
    _seam_check(curve, length, nv, rows, osc)
    _, _, bv = _seam_engine(engines, curve, length)
    assert bv.wip_verifier_workspace_bytes(SMALL_COUNT, nv) > 0 and bv.wip_verifier_workspace_bytes(SMALL_COUNT, nv + 1) == 0
    with pytest.raises(B.BppError) as ei:
        _seam_run(torch, engines, curve, length, nv + 1, S.seam_rows(curve, length, nv + 1, 2, 10))
    assert ei.value.code == -1


@pytest.mark.parametrize("curve,zero_of", [("secp256k1", lambda r: 0), ("bls12_381", lambda r: 2 * r)])
def test_seam_zero_y_is_invalid_and_alone(curve, zero_of):
    """valid proofs from the engine's own prover: with y = 0 (mod r) at verification one proof keeps the documented verdict 1,
    its scalars are the closed forms' (inv0), and its neighbours' verdicts, scalars and results do not move"""
    torch = need_gpu()
    import test_gpu_wip as TW
    cx = TW.Ctx(curve, 8, 1, 5)
    k, nv, count, p = cx.k, 1, 9, 7
    cs, V = TW._sweep_cases(cx, nv, count, 99)
    rec, sc, _ = TW._prove_device(torch, cx, cs["a"], cs["b"], cs["y"], cs["gamma"], nv)
    rec[:, 0] = cx.wire(cs["Ap"])
    rec[:, 3 + 2 * k:] = cx.wire(V)
    ok0, osc0, ores0 = TW._verify_device(torch, cx, rec, sc, cs["y"], cs["stm"], nv)
    assert ok0.tolist() == [0] * count
    y = list(cs["y"])
    y[p] = zero_of(cx.r)
    ok, osc, ores = TW._verify_device(torch, cx, rec, sc, y, cs["stm"], nv)
    assert ok.tolist() == [1 if i == p else 0 for i in range(count)]
    others = [i for i in range(count) if i != p]
    assert np.array_equal(osc[others], osc0[others]) and np.array_equal(ores[others], ores0[others])
    import oracle as O
    want = S.seam_scalars_direct(curve, cx.length, 0, cs["stm"][p], 99, [7] * k, O.wire_to_scalars(sc[p]))
    assert np.array_equal(osc[p], S.to_wire(want))
    cx.bv.close()
