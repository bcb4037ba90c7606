"""-m gpu: the verifier's MulVec back end (csrc/impl_verify.hpp VerifyImpl::run_stage: k_var_digits, k_var_tables,
k_var_windows, the four Horner forms and the fixed-generator body of k_fixed_msm, k_partials_fold, k_finalize /
k_finalize_tree) on CHOSEN scalars and points, through bpp_debug_verifier_mulvec.

Every case of tests/mulvec_cases.py GPU_CASES builds one small verifier and holds, for ALL records of every call, the
verdict word to E != 0 and the result point to the wire form of E g, where E is the big-integer sum of scalar x discrete
log the builder computed (exact: wire results are canonical affine).  The launch geometry the hook reports must be the one
the case names, so that a change to horner_form or blocks_per_proof cannot silently drop a path.  Each case makes one call
over the cycle of record classes (several at counts below the number of classes) and then sweeps the single non-zero term
-- scalar 1 and r - 1 -- over all N terms at the same count, which is what pins the maps from term to generator to table
row.  One shape per curve runs over hashed points, against the naive MulVec (bpp_msm_batch) and the CPU oracle."""

import ctypes

import numpy as np
import pytest

import mulvec_cases as M
import oracle as O
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu

DISTINCT_PER_CLASS = 32   # a call longer than this many cycles of the classes repeats its records


def _case_id(t):
    return "%s-%dx%d-c%d-count%d-view%d" % t[:6]


@pytest.fixture(scope="module")
def engines():
    """verifiers by (curve, n, m, window_bits), built on first use and closed with the module"""
    torch = need_gpu()
    import bulletproofsplus_amd as B
    made, ariths = {}, {}

    def get(cname, n, m, c, key="new"):
        k = (cname, n, m, c, key)
        if k not in made:
            a = ariths.setdefault(cname, B.Arith.init(cname))
            pk = B.PublicKey.new(a, n * m) if key == "new" else B.PublicKey.hashed(a, n * m, b"mulvec back end")
            made[k] = (a, pk, B.BatchVerifier(pk, n, m, window_bits=c))
        return made[k]

    yield torch, B, get
    for _, _, bv in made.values():
        bv.close()


def _hook(torch, bv, m_view, records, scalars):
    """one call of the hook -> (ok (count,) u32, result (count, PW) u64, [form, blocks per proof])"""
    from bulletproofsplus_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    count, PW = records.shape[0], records.shape[2]
    assert scalars.shape[0] == count and records.dtype == np.uint64 and scalars.dtype == np.uint64
    d_pts = torch.from_numpy(np.ascontiguousarray(records).view(np.int64)).to(dev)
    d_sc = torch.from_numpy(np.ascontiguousarray(scalars).view(np.int64)).to(dev)
    d_ok = torch.full((count,), 7, dtype=torch.int32, device=dev)
    d_res = torch.full((count, PW), -1, dtype=torch.int64, device=dev)
    wsb = lib.bpp_debug_verifier_mulvec_workspace_bytes(bv.handle, count, m_view)
    assert wsb > 0
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    geo = np.zeros(2, dtype=np.uint32)
    _lib.check(lib.bpp_debug_verifier_mulvec(bv.handle, m_view, d_pts.data_ptr(), d_sc.data_ptr(), count, d_ok.data_ptr(),
                                             d_ws.data_ptr(), wsb, d_res.data_ptr(), geo.ctypes.data_as(ctypes.c_void_p),
                                             torch.cuda.current_stream().cuda_stream), "bpp_debug_verifier_mulvec")
    torch.cuda.synchronize()
    return d_ok.cpu().numpy().astype(np.uint32), d_res.cpu().numpy().view(np.uint64), geo.tolist()


def _check(b, idx, ok, res, what):
    """every record of a call against the builder's answer; idx: the builder's record behind each record of the call"""
    want_ok, want_res = b.expect_ok[idx], b.expect_result[idx]
    bad = [i for i in range(len(idx)) if ok[i] != want_ok[i] or not np.array_equal(res[i], want_res[i])]
    assert not bad, "%s: %d records differ, first %s" % (
        what, len(bad), [(i, b.cls[idx[i]], b.note[idx[i]], int(ok[i]), int(want_ok[i])) for i in bad[:8]])


@pytest.mark.parametrize("case", M.GPU_CASES, ids=_case_id)
def test_back_end_on_chosen_scalars_and_points(case, engines):
    cname, n, m, c, count, m_view, form, blocks = case
    torch, B, get = engines
    a, pk, bv = get(cname, n, m, c)
    mp = m_view or m                                      # the m of the pass
    gh, G, H = M.key_wire(cname, n * mp)
    assert np.array_equal(pk.gh, gh) and np.array_equal(pk.G_vec[:n * mp], G) and np.array_equal(pk.H_vec[:n * mp], H)
    sh = M.Shape(cname, n, mp, c)
    cl = M.classes_of(cname)
    # the cycle of classes: one call that holds them all, or -- below len(cl) records -- one call per class offset
    if count >= len(cl):
        b = M.batch(cname, n, mp, c, min(count, DISTINCT_PER_CLASS * len(cl)))
        calls = [(b, np.arange(count) % len(b.cls))]
        assert set(b.cls) == set(cl)
    else:
        calls = [(M.batch(cname, n, mp, c, count, offset=off), np.arange(count)) for off in range(0, len(cl), count)]
        assert {x for bb, _ in calls for x in bb.cls} == set(cl)
    # the sweep of the single non-zero term over all N terms, both signs, at the same count
    for off in range(0, 2 * sh.N, count):
        bb = M.batch(cname, n, mp, c, min(count, 2 * sh.N), offset=off, classes=("one_hot",))
        calls.append((bb, np.arange(count) % len(bb.cls)))
    nsweep = -(-2 * sh.N // count)
    swept = {(bb.note[i], bb.scalars_int[i][bb.note[i]]) for bb, idx in calls[-nsweep:] for i in idx}
    assert swept == {(t, s) for t in range(sh.N) for s in (1, sh.r - 1)}
    for bb, idx in calls:
        ok, res, geo = _hook(torch, bv, m_view, bb.records[idx], bb.scalars[idx])
        assert geo == [form, blocks], "launch geometry %s, the case names %s" % (geo, [form, blocks])
        _check(bb, idx, ok, res, _case_id(case))


@pytest.mark.parametrize("case", M.HASHED_CASES, ids=lambda t: "%s-%dx%d-c%d-count%d" % t)
def test_back_end_over_hashed_points_against_the_naive_mulvec(case, engines):
    """discrete logs nobody knows: the reference is the naive MulVec of the same terms -- bpp_msm_batch (double-and-add per
    term: no tables, no split, no lazy additions) for every record, the CPU oracle for the first eight"""
    cname, n, m, c, count = case
    torch, B, get = engines
    a, pk, bv = get(cname, n, m, c, key="hashed")
    other = B.PublicKey.hashed(a, 64, b"mulvec proof points")
    pool = np.ascontiguousarray(other.G_vec[:M.POOL_SIZE]).copy()
    pool[M.POOL_G0] = pk.G_vec[0]
    b = M.batch(cname, n, m, c, count, hashed=True, pool_wire=pool)
    sh = b.shape
    assert set(b.cls) == set(M.classes_of(cname, hashed=True))
    ok, res, geo = _hook(torch, bv, 0, b.records, b.scalars)
    assert geo == [3, 1]
    pts = np.concatenate([M.mulvec_points(sh, pk.gh, pk.G_vec, pk.H_vec, b.records[i]) for i in range(count)])
    naive = B.msm_batch(a, b.scalars.reshape(-1, 4), pts, [sh.N] * count)
    for i in range(count):
        assert np.array_equal(res[i], naive[i]), (i, b.cls[i], b.note[i])
        assert int(ok[i]) == (0 if int(naive[i][2 * sh.L]) else 1), (i, b.cls[i])
    assert ok[b.cls.index("all_zero")] == 0 and ok[b.cls.index("random")] == 1
    for i in range(8):
        p = pts[i * sh.N:(i + 1) * sh.N]
        if cname == "ed25519":
            want = O.point_to_wire(2, M._group(cname).msm(b.scalars_int[i], O.wire_to_points(2, p)))
        else:
            want = O.msm(sh.cid, b.scalars[i], p)
        assert np.array_equal(res[i], want), (i, b.cls[i])


def test_hook_refuses_a_short_workspace_and_a_view_that_is_none(engines):
    from bulletproofsplus_amd import _lib
    lib = _lib.lib()
    torch, B, get = engines
    a, pk, bv = get("secp256k1", 4, 8, 7)
    dev = torch.device("cuda:0")
    b = M.batch("secp256k1", 4, 8, 7, 3)
    d_pts = torch.from_numpy(b.records.view(np.int64)).to(dev)
    d_sc = torch.from_numpy(b.scalars.view(np.int64)).to(dev)
    d_ok = torch.full((3,), 7, dtype=torch.int32, device=dev)
    d_res = torch.full((3, b.shape.PW), -1, dtype=torch.int64, device=dev)
    wsb = lib.bpp_debug_verifier_mulvec_workspace_bytes(bv.handle, 3, 0)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    geo = np.full(2, 0x77777777, dtype=np.uint32)
    pg = geo.ctypes.data_as(ctypes.c_void_p)
    args = (d_pts.data_ptr(), d_sc.data_ptr(), 3, d_ok.data_ptr(), d_ws.data_ptr())
    assert lib.bpp_debug_verifier_mulvec(bv.handle, 0, *args, wsb - 1, d_res.data_ptr(), pg, None) < 0
    assert "workspace too small" in lib.bpp_last_error().decode()
    for mv in (3, 8, 16):
        assert lib.bpp_debug_verifier_mulvec_workspace_bytes(bv.handle, 3, mv) == 0
        assert lib.bpp_debug_verifier_mulvec(bv.handle, mv, *args, wsb, d_res.data_ptr(), pg, None) < 0
        assert "m_view" in lib.bpp_last_error().decode()
    torch.cuda.synchronize()
    assert (d_ok.cpu().numpy() == 7).all() and (d_res.cpu().numpy() == -1).all() and (geo == 0x77777777).all()
    # a view needs less than the verifier's own shape, and the hook takes exactly what it asks for
    assert 0 < lib.bpp_debug_verifier_mulvec_workspace_bytes(bv.handle, 3, 4) < wsb
