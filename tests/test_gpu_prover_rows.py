"""-m gpu: the batched prover's scalar stage -- k_pb_init, k_pb_round, k_pb_final (csrc/prover_batch.hpp), whole, through
bpp_debug_prover_scalars (csrc/tu_debug.hip: ProveBatchImpl::prove_batch_device's literal path with a challenge block per
proof) -- on the rows of tests/prover_rows.py: chosen challenges, witnesses and blinding at every k from 0 to 12.

Expected values are model A of prover_rows.py alone (the reference's direction, generators folded every round, in big
integers; tests/test_prover_rows_cpu.py holds it against the closed forms, against recover_rows and against pyref).  EVERY
scalar of EVERY virtual proof and every r', s', delta' is compared, bit for bit; the outputs sit in guard words.
BPP_PROVE_AMOUNT64 is an argument of the call, so the rows of a shape go in two calls: the rows without the flag, then the
rows with it.  A row whose blinding is the literals travels in such a call as the literal values written out; the literals
as a null pointer, with null challenges, have a call of their own.

The public entries are then tied to the hook: what the transcript halves (PB_PRE / PB_POST) prove from a chosen d_blinding,
the whole kernels must prove again from the same inputs and the challenges the transcript drew.

Verifiers are made with window_bits 3, as in tests/test_gpu_recover_rows.py.

Wall time on one MI355X: the module's 62 tests in 14 s, 1.5 s of it the setup before the first test.  Slowest calls:
test_points_on_edwards25519_equal_pyref at (2,4) and (8,1) 1.9 s each (pyref's group law in Python), the oracle MulVecs at
mn = 32 0.8 s, every sweep of a shape's rows under 0.35 s ((64,64), three rows of 24 MB)."""

import ctypes

import numpy as np
import pytest

import oracle as O
import prover_rows as PR
import pyref as P
import recover_rows as RR
from gpu_util import need_gpu, run_verifier_device

pytestmark = pytest.mark.gpu

WINDOW_BITS = 3
GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)
AMOUNT64 = 0x100


@pytest.fixture(scope="module")
def engines():
    """(arith, key, verifier) by (curve, n, m), built on first use and closed with the module"""
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


def _inputs(rows, null_ch=False, null_blind=False):
    values = np.array([row.values for row in rows], dtype=np.uint64)
    gammas = PR.to_wire([g for row in rows for g in row.gammas])
    blind = None if null_blind else PR.to_wire([x for row in rows for x in row.blind_values()])
    ch = None if null_ch else PR.to_wire([x for row in rows for x in row.ch_values()])
    return values, gammas, blind, ch


def _hook_rc(bv, m_view, flags, values, gammas, blind, ch, count, vps, s3, pts):
    from bulletproofsplus_amd import _lib
    return _lib.lib().bpp_debug_prover_scalars(bv.handle, m_view, flags, _ptr(values), _ptr(gammas), _ptr(blind), _ptr(ch), count,
                                               _ptr(vps), _ptr(s3), _ptr(pts))


def _hook(bv, m_view, rows, want_points=False, null_ch=False, null_blind=False):
    """one call over rows of one shape and one flag -> (vps (count, 2k + 3 + m, N, 4), triples (count, 3, 4), points or None)"""
    from bulletproofsplus_amd import _lib
    n, m, k, flag = rows[0].n, rows[0].m, rows[0].k, rows[0].flag
    assert all((row.n, row.m, row.flag) == (n, m, flag) for row in rows)
    if null_ch or null_blind:
        assert all((row.ch is None or not null_ch) and (row.blind is None or not null_blind) for row in rows)
    count = len(rows)
    vps = np.full((count, PR.num_vps(k, m), PR.n_scalars(n, m), 4), GUARD, dtype=np.uint64)
    s3 = np.full((count + 1, 3, 4), GUARD, dtype=np.uint64)
    pts = np.full((count + 1, 3 + 2 * k + m, bv.arith.PW), GUARD, dtype=np.uint64) if want_points else None
    rc = _hook_rc(bv, m_view, AMOUNT64 if flag else 0, *_inputs(rows, null_ch, null_blind), count, vps, s3, pts)
    _lib.check(rc, "bpp_debug_prover_scalars")
    assert (s3[count] == GUARD).all() and (pts is None or (pts[count] == GUARD).all())
    return vps, s3[:count], None if pts is None else pts[:count]


def _want(rows):
    exp = [PR.model_a(row) for row in rows]
    return exp, np.stack([PR.vps_wire(row, pts) for row, (pts, _) in zip(rows, exp)]), \
        PR.to_wire([x for _, triple in exp for x in triple]).reshape(len(rows), 3, 4)


def _assert_rows(got_vps, got_s3, rows, what):
    _, want_vps, want_s3 = _want(rows)
    if not np.array_equal(got_vps, want_vps):
        bad = np.argwhere((got_vps != want_vps).any(axis=3))
        raise AssertionError("%s: %d scalars differ, rows %s; first (proof, row, virtual proof, term) %s" % (
            what, len(bad), sorted({rows[i].name for i in set(bad[:, 0].tolist())}),
            [(int(i), rows[i].name, int(v), int(t)) for i, v, t in bad[:8]]))
    bad = [rows[i].name for i in range(len(rows)) if not np.array_equal(got_s3[i], want_s3[i])]
    assert not bad, "%s: r', s', delta' differ in rows %s" % (what, bad)


def _by_flag(rows):
    return [part for part in ([row for row in rows if not row.flag], [row for row in rows if row.flag]) if part]


def _engine_of(engines, cname, n, m, cap_n1=64, cap_n64=64):
    """the verifier and the view that run shape (n, m): (1, m) as a view of (1,64), (64, m) of (64, cap_n64), (n, 1) its own"""
    if n == 1:
        return engines(cname, 1, cap_n1)[2], (0 if m == cap_n1 else m)
    if n == 64:
        return engines(cname, 64, cap_n64)[2], (0 if m == cap_n64 else m)
    assert m == 1
    return engines(cname, n, 1)[2], 0


def _sweep(engines, cname, n, m, cap_n64=64):
    bv, m_view = _engine_of(engines, cname, n, m, cap_n64=cap_n64)
    rows = PR.shape_rows(cname, n, m)
    assert {row.name for row in rows} == set(PR.row_names(n, m))
    for part in _by_flag(rows):
        vps, s3, _ = _hook(bv, m_view, part)
        _assert_rows(vps, s3, part, "%s (%d,%d) view %d flag %d" % (cname, n, m, m_view, part[0].flag))


# ---- 1. the hook against model A ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(7))
@pytest.mark.parametrize("cname", PR.CURVES)
def test_every_row_at_k_0_to_6(engines, cname, k):
    """(2^k, 1) on a verifier of its own -- (64,1) as the view 1 of (64,64) --, (1, 2^k) as a view of (1,64): 33 rows a shape,
    31 and 2 proofs a call, a challenge block and 5 + 2k blinding scalars per proof"""
    shapes = RR.shapes(k)
    assert (1 << k, 1) in shapes and (k == 0 or (1, 1 << k) in shapes)
    for n, m in shapes:
        _sweep(engines, cname, n, m)


@pytest.mark.parametrize("k", range(7, 13))
def test_every_row_at_k_7_to_12_on_the_largest_verifier(engines, k):
    """(64, 2) .. (64, 32) as views of the (64,64) verifier, then its own shape; from k = 9 three rows a shape"""
    (shape,) = RR.shapes(k)
    assert shape == (64, 1 << (k - 6))
    _sweep(engines, "bls12_381", *shape)


@pytest.mark.parametrize("cname", ("secp256k1", "ed25519"))
def test_every_row_at_64_4_as_a_verifier_of_its_own(engines, cname):
    _sweep(engines, cname, 64, 4, cap_n64=4)


def _with(row, **kw):
    d = dict(row.__dict__)
    d.update(kw)
    return PR.Row(**d)


@pytest.mark.parametrize("cname,n,m,m_own", [("bls12_381", 8, 1, 1), ("secp256k1", 1, 8, 64), ("ed25519", 64, 2, 4)])
def test_one_proof_and_the_literals_as_null_pointers(engines, cname, n, m, m_own):
    """count 1; then null challenges (one block shared at stride 0) with null blinding, null challenges alone, null blinding
    alone -- the witnesses of five rows, the literal values [7, 7 | 12, 23, 99, 7..] and [7 | 33, 33, 44, 88, 123, 4.., 5..]
    from prover_rows"""
    bv = engines(cname, n, m_own)[2]
    m_view = 0 if m == m_own else m
    rows = PR.shape_rows(cname, n, m)
    one = [row for row in rows if row.name == "top(3)"]
    vps, s3, _ = _hook(bv, m_view, one)
    _assert_rows(vps, s3, one, "count 1")
    pick = [row for row in rows if row.name in ("literal", "identity", "amount(max)", "gamma(-1)", "amount_i32_negative")]
    assert len(pick) == 5
    for null_ch, null_blind in ((True, True), (True, False), (False, True)):
        part = [_with(row, **dict(([("ch", None)] if null_ch else []) + ([("blind", None)] if null_blind else []))) for row in pick]
        vps, s3, _ = _hook(bv, m_view, part, null_ch=null_ch, null_blind=null_blind)
        _assert_rows(vps, s3, part, "null challenges %d, null blinding %d" % (null_ch, null_blind))


# ---- 2. out_points: the prover's own MulVec over every virtual proof ------------------------------------------------------------
POINT_ROWS = ("random", "identity", "zero_a(z=0)", "zero_a(z=1)", "amount64(max)", "blind(zero)", "top(0)", "literal")


def _oracle_points(cname, n, m, exp):
    """[count][3 + 2k + m] wire points: the C oracle's MulVec of model A's coefficients over PublicKey::new(n m)"""
    curve = O.CURVE_IDS[cname]
    opk = O.PublicKey(curve, n * m)
    gens = np.concatenate([opk.gh, opk.G, opk.H])
    inf = O.point_to_wire(curve, None)
    out = []
    for pts, _ in exp:
        out.append([O.msm(curve, PR.to_wire(p.values()), gens[list(p.keys())]) if p else inf for p in pts])
    return np.array(out, dtype=np.uint64)


def _pyref_points(cname, n, m, exp):
    G = P.make_group(cname, False)
    ppk = P.PublicKey(G, n * m)
    gens = [ppk.g, ppk.h] + list(ppk.G_vec) + list(ppk.H_vec)
    out = []
    for pts, _ in exp:
        row = []
        for p in pts:
            mv = P.MulVec(G)
            mv.add_scalars(list(p.values()))
            mv.add_points([gens[f] for f in p])
            row.append(mv.calculate())
        out.append(row)
    return out


def _record_order(k, m, vps_points):
    """virtual-proof numbering -> the record [A, wip.A, wip.B, L.., R..] and the commitments behind it"""
    return ([vps_points[0], vps_points[2 * k + 1], vps_points[2 * k + 2]] + [vps_points[1 + 2 * t] for t in range(k)] +
            [vps_points[2 + 2 * t] for t in range(k)] + list(vps_points[2 * k + 3:]))


def _point_rows(cname, n, m):
    by_name = {row.name: row for row in PR.shape_rows(cname, n, m)}
    rows = [by_name[name] for name in POINT_ROWS]
    assert any(all(p == {} for p in PR.expected(cname, n, m, row.name)[0][-m:]) for row in rows)          # identity V
    assert any(all(0 not in p for p in PR.expected(cname, n, m, row.name)[0][1:2 * row.k + 1]) for row in rows) or n * m == 1
    return rows


@pytest.mark.parametrize("n,m", [(1, 1), (2, 1), (1, 2), (8, 1), (2, 4), (32, 1), (4, 8)])
@pytest.mark.parametrize("cname", ("bls12_381", "secp256k1"))
def test_points_equal_the_oracle_mulvec_of_model_a(engines, cname, n, m):
    """mn <= 32: the record and the commitments as wire points; the identity commitment and the zero a vector among them"""
    bv = engines(cname, n, m)[2]
    for part in _by_flag(_point_rows(cname, n, m)):
        vps, s3, pts = _hook(bv, 0, part, want_points=True)
        _assert_rows(vps, s3, part, "%s (%d,%d)" % (cname, n, m))
        exp = [PR.expected(cname, n, m, row.name) for row in part]
        want = np.stack([np.stack(_record_order(part[0].k, m, list(w))) for w in _oracle_points(cname, n, m, exp)])
        assert pts.shape == want.shape
        bad = np.argwhere((pts != want).any(axis=2))
        assert not len(bad), [(part[i].name, int(v)) for i, v in bad[:8]]
        ident = [i for i, row in enumerate(part) if row.name == "identity"]
        assert all(O.wire_to_point(O.CURVE_IDS[cname], pts[i, -1]) is None for i in ident)


@pytest.mark.parametrize("n,m", [(1, 1), (2, 1), (1, 4), (8, 1), (2, 4)])
def test_points_on_edwards25519_equal_pyref(engines, n, m):
    cname = "ed25519"
    bv = engines(cname, n, m)[2]
    rows = [row for row in _point_rows(cname, n, m) if row.name in ("random", "identity", "zero_a(z=1)", "amount64(max)")]
    for part in _by_flag(rows):
        vps, s3, pts = _hook(bv, 0, part, want_points=True)
        _assert_rows(vps, s3, part, "%s (%d,%d)" % (cname, n, m))
        exp = [PR.expected(cname, n, m, row.name) for row in part]
        want = [_record_order(part[0].k, m, w) for w in _pyref_points(cname, n, m, exp)]
        got = [O.wire_to_points(O.ED25519, pts[i]) for i in range(len(part))]
        assert got == want, [row.name for row, g, w in zip(part, got, want) if g != w]


# ---- 3. what the hook refuses ------------------------------------------------------------------------------------------------
def test_hook_refuses_bad_arguments(engines):
    from bulletproofsplus_amd import _lib
    bv = engines("secp256k1", 1, 64)[2]
    rows = [row for row in PR.shape_rows("secp256k1", 1, 8) if not row.flag][:2]
    values, gammas, blind, ch = _inputs(rows)
    vps = np.full((2, PR.num_vps(3, 8), PR.n_scalars(1, 8), 4), GUARD, dtype=np.uint64)
    s3 = np.full((2, 3, 4), GUARD, dtype=np.uint64)
    for m_view in (3, 64, 128):
        assert _hook_rc(bv, m_view, 0, values, gammas, blind, ch, 2, vps, s3, None) == -1
        assert "m_view" in _lib.lib().bpp_last_error().decode()
    assert _hook_rc(bv, 8, 1, values, gammas, blind, ch, 2, vps, s3, None) == -1          # a flag that is not AMOUNT64
    assert _hook_rc(bv, 8, 0, None, gammas, blind, ch, 2, vps, s3, None) == -1
    assert _hook_rc(bv, 8, 0, values, gammas, blind, ch, 2, None, s3, None) == -1
    assert _hook_rc(bv, 8, 0, values, gammas, blind, ch, 2049, vps, s3, None) == -1       # beyond one chunk
    assert "chunk" in _lib.lib().bpp_last_error().decode()
    assert _hook_rc(bv, 8, 0, values, gammas, blind, ch, 0, vps, s3, None) == 0           # count 0: nothing is written
    assert (vps == GUARD).all() and (s3 == GUARD).all()


def test_the_abi_still_refuses_blinding_without_the_transcript(engines):
    torch = need_gpu()
    import bulletproofsplus_amd as B
    _, _, bv = engines("secp256k1", 8, 2)
    rows = [row for row in PR.shape_rows("secp256k1", 8, 2) if not row.flag][:2]
    with pytest.raises(B.BppError) as ei:
        _prove_mixed(torch, bv, rows, transcript=False)
    assert ei.value.code == -1


# ---- 4. the halves and the whole ----------------------------------------------------------------------------------------------
def _dev(torch, x):
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.uint8).reshape(-1)).to(torch.device("cuda:0"))


def _host(t, shape):
    return t.cpu().numpy().view(np.uint64).reshape(shape)


def _nv(n, m):
    return 3 + 2 * RR.log2(n * m) + m


def _prove_fs(torch, bv, rows):
    """bpp_range_prove_batch_fs_device with d_blinding = the rows' -> (records+commitments (count, NV, PW), triples,
    challenges (count, 3 + k, 4), derive_challenges_device of the records)"""
    n, m, k, count, PW = rows[0].n, rows[0].m, rows[0].k, len(rows), bv.arith.PW
    values, gammas, blind, _ = _inputs(rows)
    d_v, d_g, d_b = _dev(torch, values), _dev(torch, gammas), _dev(torch, blind)
    d_p = torch.full((count * (3 + 2 * k) * PW * 8,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_V = torch.full((count * m * PW * 8,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_s = torch.full((count * 96,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_c = torch.full((count * (3 + k) * 32,), 0x5a, dtype=torch.uint8, device="cuda:0")
    wsb = bv.prover_workspace_bytes(count)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    bv.prove_batch_device(d_v.data_ptr(), d_g.data_ptr(), count, d_p.data_ptr(), d_s.data_ptr(), d_V.data_ptr(), d_ws.data_ptr(),
                          wsb, st, transcript=True, d_out_challenges=d_c.data_ptr(), d_blinding=d_b.data_ptr())
    torch.cuda.synchronize()
    rec = np.concatenate([_host(d_p, (count, 3 + 2 * k, PW)), _host(d_V, (count, m, PW))], axis=1)
    d_rec = _dev(torch, rec)
    d_c2 = torch.zeros_like(d_c)
    bv.derive_challenges_device(d_rec.data_ptr(), count, d_c2.data_ptr(), st)
    torch.cuda.synchronize()
    return rec, _host(d_s, (count, 3, 4)), _host(d_c, (count, 3 + k, 4)), _host(d_c2, (count, 3 + k, 4))


def _rows_with_challenges(rows, ch):
    return [_with(row, ch=O.wire_to_scalars(c)) for row, c in zip(rows, ch)]


EDGE_NAMES = ("random", "amount(0)", "amount(1)", "amount(max)", "amount(half)", "identity", "gamma(0)", "gamma(1)", "gamma(-1)",
              "blind_edges(0)", "blind_edges(1)", "blind_edges(2)", "blind(zero)", "blind(literal)", "amount_i32_negative")


@pytest.mark.parametrize("cname,n,m", [("bls12_381", 8, 2), ("secp256k1", 16, 1), ("ed25519", 4, 4)])
def test_transcript_halves_equal_the_whole_kernels_on_their_challenges(engines, cname, n, m):
    """PB_PRE / PB_POST under the transcript, blinding from a buffer of 0 / 1 / r - 1, zeros and the literals written out,
    the edge amounts and gammas: d_out_challenges is what the verifier derives, and the whole kernels, given those
    challenges, leave the same record, commitments and triple -- and model A's scalars.  The verifier accepts every proof
    whose amounts are in range."""
    torch = need_gpu()
    bv = engines(cname, n, m)[2]
    by_name = {row.name: row for row in PR.shape_rows(cname, n, m)}
    rows = [by_name[name] for name in EDGE_NAMES]
    rec, s3, ch, derived = _prove_fs(torch, bv, rows)
    assert np.array_equal(ch, derived)
    r = rows[0].r
    assert all(0 < x < r for x in O.wire_to_scalars(ch))
    again = _rows_with_challenges(rows, ch)
    vps, s3_hook, pts = _hook(bv, 0, again, want_points=True)
    _assert_rows(vps, s3_hook, again, "%s (%d,%d) on the transcript's challenges" % (cname, n, m))
    assert np.array_equal(pts, rec) and np.array_equal(s3_hook, s3)
    ok, _, _ = run_verifier_device(torch, bv, rec, s3, want_scalars=False, want_result=False, challenges=ch)
    in_range = [all(v < 1 << n and PR.i32(v) == v for v in row.values) for row in rows]
    assert ok.tolist() == [0 if x else 1 for x in in_range] and in_range.count(False) == 1


def _prove_mixed(torch, bv, rows, transcript=True, amount64=True):
    """bpp_range_prove_batch_mixed_device over rows of shapes (n, m_i) with packed d_blinding -> (packed records, triples,
    packed challenges, device buffers)"""
    n, PW, ms = rows[0].n, bv.arith.PW, [row.m for row in rows]
    values = np.array([v for row in rows for v in row.values], dtype=np.uint64)
    gammas = PR.to_wire([g for row in rows for g in row.gammas])
    blind = PR.to_wire([x for row in rows for x in row.blind_values()])
    d_v, d_g, d_b = _dev(torch, values), _dev(torch, gammas), _dev(torch, blind)
    npts, nch = sum(_nv(n, m) for m in ms), sum(3 + RR.log2(n * m) for m in ms)
    d_p = torch.full((npts * PW * 8,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_s = torch.full((len(ms) * 96,), 0x5a, dtype=torch.uint8, device="cuda:0")
    d_c = torch.full((nch * 32,), 0x5a, dtype=torch.uint8, device="cuda:0")
    wsb = bv.prover_mixed_workspace_bytes(ms)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    bv.prove_mixed_device(d_v.data_ptr(), d_g.data_ptr(), ms, d_p.data_ptr(), d_s.data_ptr(), d_ws.data_ptr(), wsb,
                          torch.cuda.current_stream().cuda_stream, transcript=transcript, d_out_challenges=d_c.data_ptr(),
                          d_blinding=d_b.data_ptr(), amount64=amount64)
    torch.cuda.synchronize()
    return _host(d_p, (npts, PW)), _host(d_s, (len(ms), 3, 4)), _host(d_c, (nch, 4)), d_p, d_s, d_c


def test_a_mixed_block_view_equals_the_whole_kernels(engines):
    """(64,2) with BPP_PROVE_AMOUNT64: proofs of one and of two amounts interleaved -- 2^64 - 1, 2^63, 0 with gamma 0, the
    blinding edges -- through the mixed device entry; every proof again through the hook at its own view"""
    torch = need_gpu()
    cname, n = "bls12_381", 64
    bv = engines(cname, n, 2)[2]
    names = ("amount64(max)", "amount64(2^63)", "identity", "blind_edges(1)", "blind(zero)", "amount(max)")
    rows = []
    for name in names:
        for m in (1, 2):
            rows.append(_with({row.name: row for row in PR.shape_rows(cname, n, m)}[name], flag=True))
    rows = rows[1:] + rows[:1]       # starts with m = 2, ends with m = 1
    ms = [row.m for row in rows]
    pts, s3, ch, d_p, d_s, d_c = _prove_mixed(torch, bv, rows)
    wsb = bv.mixed_workspace_bytes(ms)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    d_c2 = torch.zeros_like(d_c)
    st = torch.cuda.current_stream().cuda_stream
    bv.derive_challenges_mixed_device(d_p.data_ptr(), ms, d_c2.data_ptr(), d_ws.data_ptr(), wsb, st)
    torch.cuda.synchronize()
    assert torch.equal(d_c, d_c2)
    po = np.concatenate([[0], np.cumsum([_nv(n, m) for m in ms])]).astype(int)
    co = np.concatenate([[0], np.cumsum([3 + RR.log2(n * m) for m in ms])]).astype(int)
    for m in (1, 2):
        idx = [i for i, x in enumerate(ms) if x == m]
        again = [_with(rows[i], ch=O.wire_to_scalars(ch[co[i]:co[i + 1]])) for i in idx]
        vps, s3_hook, hp = _hook(bv, 0 if m == 2 else 1, again, want_points=True)
        _assert_rows(vps, s3_hook, again, "view %d" % m)
        assert np.array_equal(hp, np.stack([pts[po[i]:po[i + 1]] for i in idx])) and np.array_equal(s3_hook, s3[idx])
    d_ok = torch.full((len(ms),), 7, dtype=torch.int32, device="cuda:0")
    bv.run_mixed_device(d_p.data_ptr(), d_s.data_ptr(), ms, d_ok.data_ptr(), d_ws.data_ptr(), wsb, st, d_challenges=d_c.data_ptr())
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [0] * len(ms)


@pytest.mark.parametrize("cname,version", [("bls12_381", 1), ("bls12_381", 2), ("secp256k1", 1), ("secp256k1", 2), ("ed25519", 1)])
def test_identity_commitment_and_all_ones_amount_as_bytes(engines, cname, version):
    """V = 0 g + 0 h, the point at infinity, and the amount 2^64 - 1 through prove_serialized_mixed and the serialized verify
    call, literal and transcript mode: every container verifies, and a flipped byte of a commitment does not"""
    need_gpu()
    bv = engines(cname, 64, 2)[2]
    top = (1 << 64) - 1
    values = [[0], [top, 1 << 63], [0, 0], [top], [0, top]]
    gammas = [[0], [5, 0], [0, 0], [rows_r(cname) - 1], [0, 1]]
    for transcript in (False, True):
        proofs, cms, ms = bv.prove_serialized_mixed(values, gammas, transcript=transcript, uncompressed=version == 2,
                                                    amount64=True)
        assert ms.tolist() == [1, 2, 2, 1, 2]
        ok = bv.verify_serialized_mixed(proofs, cms, ms, transcript=transcript, uncompressed=version == 2)
        assert ok.tolist() == [0] * 5, (transcript, ok.tolist())
        # without the flag the commitment of 2^64 - 1 is -1 g: other bytes, and its proof no longer verifies against them
        p2, c2, _ = bv.prove_serialized_mixed(values, gammas, transcript=transcript, uncompressed=version == 2)
        assert c2 != cms
        ok2 = bv.verify_serialized_mixed(proofs, c2, ms, transcript=transcript, uncompressed=version == 2)
        assert ok2.tolist()[0] == 0 and ok2.tolist()[2] == 0 and 0 not in (ok2.tolist()[1], ok2.tolist()[3], ok2.tolist()[4])


def rows_r(cname):
    return PR.ORDER[cname]
