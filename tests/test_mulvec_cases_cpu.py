"""CPU: the case builder of the back-end tests (tests/mulvec_cases.py) is itself right, and the hook it feeds
(bpp_debug_verifier_mulvec) turns usage errors into return codes that write nothing.

Per pass shape of the GPU test: every scalar is canonical, every record class occurs, the one-hot sweep reaches every term
of the MulVec (the left-over generators of the NF = 258 shapes included), cancel / near_miss records sum to 0 / 1, the
`digits` scalars recode to the digits they claim (recomputed here from c, W and half; on BLS12-381 from the layout rule of
csrc/fixed_glv.hpp, which is also held to the host build of that header), and for a sample of records of every class
E g -- the builder's big-integer answer -- is the MulVec the oracle computes term by term over the same points and scalars.
No GPU needed: nothing here reaches a device."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import glv_cases as GC
import mulvec_cases as M
import oracle as O
import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = M.pass_shapes()
SENTINEL = 0x7777777777777777


def _id(t):
    return "%s-%dx%d-c%d" % t


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_every_class_is_present_and_every_scalar_canonical(shape):
    cname, n, m, c = shape
    cl = M.classes_of(cname)
    assert set(cl) == set(M.CLASSES) - (set() if cname == "bls12_381" else {"z2_multiples"})
    for off in (0, 5):
        b = M.batch(cname, n, m, c, len(cl), offset=off)
        assert sorted(b.cls) == sorted(cl)           # a batch of len(classes) records holds every class, at any offset
        r = b.shape.r
        assert all(0 <= s < r for row in b.scalars_int for s in row)
        assert b.scalars.shape == (len(cl), b.shape.N, 4) and b.records.shape == (len(cl), b.shape.NV, b.shape.PW)
        assert [O.limbs_to_int(w) for w in b.scalars[3]] == b.scalars_int[3]
        for i, cls in enumerate(b.cls):
            S, sh = b.scalars_int[i], b.shape
            if cls == "all_zero":
                assert not any(S) and b.E[i] == 0 and b.expect_ok[i] == 0
            if cls == "fixed_only":
                assert not any(S[t] for t in sh.proof_terms) and all(S[t] for t in sh.fixed_terms)
            if cls == "proof_only":
                assert not any(S[t] for t in sh.fixed_terms) and all(S[t] for t in sh.proof_terms)
            if cls == "all_one":
                assert S == [1] * sh.N
            if cls == "all_minus_one":
                assert S == [r - 1] * sh.N
            if cls == "small":
                assert max(S) < 1 << 64
            if cls == "z2_multiples":
                assert all(M.balanced_split(s)[0] == 0 for s in S) and any(S)
            if cls == "cancel":
                assert b.E[i] == 0 and b.expect_ok[i] == 0 and int(b.expect_result[i][2 * sh.L]) == 1
            if cls == "near_miss":
                assert b.E[i] == 1 and b.expect_ok[i] == 1
                assert np.array_equal(b.expect_result[i], M.wire_of_dlog(cname, 1))
    # the sorted order of terms is the MulVec's: a permutation of 0 .. N - 1
    sh = b.shape
    assert sorted(sh.fixed_terms + sh.proof_terms) == list(range(sh.N))


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_one_hot_sweep_reaches_every_term(shape):
    cname, n, m, c = shape
    sh = M.Shape(cname, n, m, c)
    b = M.batch(cname, n, m, c, 2 * sh.N, classes=("one_hot",))
    seen = {}
    for i in range(2 * sh.N):
        S, t = b.scalars_int[i], b.note[i]
        assert sum(1 for s in S if s) == 1 and S[t] in (1, sh.r - 1)
        seen.setdefault(t, set()).add(S[t])
        d = b.dlogs[i][t]
        assert b.E[i] == (d if S[t] == 1 else (sh.r - d) % sh.r) and d != 0   # exactly that point, or its negative
    assert seen == {t: {1, sh.r - 1} for t in range(sh.N)}
    if sh.NF == 258:   # the two generators that are left over when 128 or 256 lanes share 258
        assert {sh.fixed_term_index(256), sh.fixed_term_index(257)} <= set(seen)
    # a sweep split over calls of any length is the same sweep
    parts = [M.batch(cname, n, m, c, 5, offset=o, classes=("one_hot",)) for o in (0, 5)]
    assert [p.scalars_int for p in parts] == [b.scalars_int[:5], b.scalars_int[5:10]]


@pytest.fixture(scope="module")
def glv_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mulvec_cases") / "bpp_fixed_glv_host_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "host", "fixed_glv_host_test.cpp")])
    return out


@pytest.mark.parametrize("cname,c", sorted({(s[0], s[3]) for s in SHAPES}))
def test_digit_scalars_recode_to_the_digits_claimed(cname, c, glv_exe):
    sh = M.Shape(cname, 2, 2, c)
    r, W = sh.r, sh.W
    ds = M.digit_scalars(cname, c)
    assert all(0 <= k < r for k, _ in ds)
    if not sh.glv:
        half = 1 << (c - 1)
        assert W == (r.bit_length() - 1) // c + 1

        def digits(k):   # v = k + bias, the signed windows below the top one, what is left in the top window
            v = k + sum(half << (c * j) for j in range(W - 1))
            return [((v >> (c * j)) % (1 << c)) - half for j in range(W - 1)] + [v >> (c * (W - 1))]

        claimed = [d for k, d in ds if d is not None and digits(k) == d]
        assert len(claimed) == sum(1 for _, d in ds if d is not None)
        below = [tuple(d[:-1]) for d in claimed]
        assert (-half,) * (W - 1) in below and (half - 1,) * (W - 1) in below
        assert tuple((-half, half - 1)[j % 2] for j in range(W - 1)) in below
        assert tuple((half - 1, -half)[j % 2] for j in range(W - 1)) in below
        assert max(d[-1] for d in claimed) == sh.top == digits(r - 1)[-1]   # the largest top digit a canonical scalar has
        assert all(-half <= x < half for d in claimed for x in d[:-1])
        return
    # the layout rule against the host build of csrc/fixed_glv.hpp
    out = subprocess.check_output([glv_exe, "layout", str(c)]).decode().splitlines()
    Wd, top, _ = (int(x) for x in out[0].split())
    wins = [tuple(int(x) for x in line.split()) for line in out[1:1 + Wd]]
    assert (Wd, top) == (W, sh.top)
    assert [w for w, _, _ in wins[:-1]] == sh.widths and [o for _, o, _ in wins] == sh.offs
    assert int(out[1 + Wd], 16) == sh.bias
    # ... and the split against the host build of csrc/ec.hpp
    lines = subprocess.check_output([glv_exe, "split"] + ["%064x" % k for k, _ in ds]).decode().splitlines()
    for (k, _), line in zip(ds, lines):
        s1, k1, s2, k2 = line.split()
        k1, k2 = int(k1, 16) * (-1 if s1 == "1" else 1), int(k2, 16) * (-1 if s2 == "1" else 1)
        assert (k1, k2) == M.balanced_split(k), hex(k)

    def digits(h):
        v = h + sum(1 << (o + w - 1) for o, w in zip(sh.offs, sh.widths))
        return [((v >> o) % (1 << w)) - (1 << (w - 1)) for o, w in zip(sh.offs, sh.widths)] + [v >> sh.offs[-1]]

    lo = tuple(-(1 << (w - 1)) for w in sh.widths)
    hi = tuple((1 << (w - 1)) - 1 for w in sh.widths)
    alt = tuple((lo[j], hi[j])[j % 2] for j in range(W - 1))
    alt2 = tuple((hi[j], lo[j])[j % 2] for j in range(W - 1))
    seen = [set(), set()]   # (digits below the top, sign) met per half
    for k, claim in ds:
        if claim is None:
            continue
        got = M.balanced_split(k)
        for h in (0, 1):
            want, d = claim[h]
            assert got[h] == want and digits(abs(want)) == d, (hex(k), h)
            seen[h].add((tuple(d[:-1]), want < 0))
    for h in (0, 1):
        for pat in (lo, hi, alt, alt2):
            assert (pat, False) in seen[h] and (pat, True) in seen[h]
    # the largest top digit a half can have: k1 reaches z^2 / 2 and k2 z^2 / 2 - 1 (test_fixed_glv_cpu.py), both among the edges
    halves = [M.balanced_split(k) for k, _ in ds]
    assert max(abs(a) for a, _ in halves) == GC.Z2 // 2 and max(abs(b) for _, b in halves) >= GC.Z2 // 2 - 1
    assert {(a > 0) - (a < 0) for a, _ in halves} == {-1, 0, 1} == {(b > 0) - (b < 0) for _, b in halves}
    grid = {0, 1, -1, GC.HALF_MAX - 1, 1 - GC.HALF_MAX, GC.HALF_MAX, -GC.HALF_MAX}
    assert {(k1 + k2 * GC.Z2) % r for k1 in grid for k2 in grid} | set(GC.edges()) <= {k for k, _ in ds}


@pytest.mark.parametrize("cname", ["bls12_381", "secp256k1", "ed25519"])
def test_nibble_scalars(cname):
    r = P.CURVES[cname]["r"]
    ns = M.nibble_scalars(cname)
    assert all(0 <= k < r for k, _ in ns)
    for k, d in ns:
        if d is not None:
            assert M.recode_nibbles(k, 65) == d and sum(x << (4 * j) for j, x in enumerate(d)) == k
    if cname == "ed25519":
        ds = [tuple(d) for _, d in ns if d is not None]
        assert (-8,) * 63 + (1, 0) in ds and (7,) * 63 + (0, 0) in ds
        assert any(d[63] != 0 for d in ds) and r - 1 in [k for k, _ in ns]
    if cname != "ed25519":
        # a batch reads the list cyclically from its start: the 36 entries that the four `nibbles` records of a 64-proof
        # 2 x 2 case (NV = 9) feed already hold all 7, all -8 and 8 * 16^j of every window j, on both halves at once
        mu, first = M.Shape(cname, 2, 2, 4).mu, {k for k, _ in ns[:36]}
        n7, n8 = int("7" * 32, 16), (1 << 128) - int("8" * 32, 16)
        assert all((h + h * mu) % r in first for h in [n7, n8] + [8 << (4 * j) for j in range(32)])
    if cname == "bls12_381":   # the device's split of a proof-point scalar is (k mod z^2, k div z^2): halves of all -8 / all 7
        halves = {(k % GC.Z2, k // GC.Z2) for k, _ in ns}
        n7, n8 = int("7" * 32, 16), (1 << 128) - int("8" * 32, 16)
        assert {(n7, n7), (n8, n8), (n7, 0), (0, n8)} <= halves
        assert all(any(h == (8 << (4 * j), 0) for h in halves) and any(h == (0, 8 << (4 * j)) for h in halves) for j in range(31))
    if cname == "secp256k1":
        lam, n7 = GC.SECP_LAMBDA, int("7" * 32, 16)
        assert {(n7 + n7 * lam) % r, (n7 - n7 * lam) % r, (-n7 + n7 * lam) % r, (-n7 - n7 * lam) % r} <= {k for k, _ in ns}


def _sample(cname, n, m, c):
    """one record of every class, then further `points` and `digits` variants: at least 16 records"""
    cl = M.classes_of(cname)
    b = M.batch(cname, n, m, c, len(cl))
    extra = M.batch(cname, n, m, c, 6, offset=len(cl), classes=("points", "digits", "nibbles"))
    return [(b, i) for i in range(len(cl))] + [(extra, i) for i in range(6)]


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_big_integer_answer_is_the_oracles_mulvec(shape):
    cname, n, m, c = shape
    sh = M.Shape(cname, n, m, c)
    gh, G, H = M.key_wire(cname, sh.mn)
    if cname != "ed25519":   # the key with known discrete logs is PublicKey::new's
        opk = O.PublicKey(sh.cid, sh.mn)
        assert np.array_equal(gh, opk.gh) and np.array_equal(G, opk.G) and np.array_equal(H, opk.H)
    sample = _sample(cname, n, m, c)
    assert len(sample) >= 16
    for b, i in sample:
        pts = M.mulvec_points(sh, gh, G, H, b.records[i])
        assert pts.shape == (sh.N, sh.PW)
        if cname == "ed25519":
            mv = P.MulVec(M._group(cname))
            mv.add_scalars(b.scalars_int[i])
            mv.add_points(O.wire_to_points(2, pts))
            got = O.point_to_wire(2, mv.calculate())
        else:
            got = O.msm(sh.cid, b.scalars[i], pts)
        assert np.array_equal(got, b.expect_result[i]), (b.cls[i], b.note[i])
        assert (int(got[2 * sh.L]) == 1) == (b.expect_ok[i] == 0)
        # the dlogs the builder summed over are those of the points it emitted
        for t in (0, 3, sh.N - 1):
            assert np.array_equal(M.wire_of_dlog(cname, b.dlogs[i][t]), pts[t])


def test_points_class_holds_what_it_claims():
    cname, n, m, c = "secp256k1", 4, 4, 7
    b = M.batch(cname, n, m, c, M.POINT_VARIANTS, classes=("points",))
    sh, k = b.shape, b.shape.k
    rec, S = b.records, b.scalars_int
    sc = lambda i, v: S[i][sh.var_term_index(v)]
    neg = lambda w: O.point_neg(sh.cid, w)
    inf = O.point_to_wire(sh.cid, None)
    assert [b.note[i] for i in range(M.POINT_VARIANTS)] == list(range(M.POINT_VARIANTS))
    assert np.array_equal(rec[0, 3], rec[0, 3 + k]) and sc(0, 3) != sc(0, 3 + k)
    assert np.array_equal(rec[1, 3], rec[1, 3 + k]) and sc(1, 3) == sc(1, 3 + k) != 0
    assert np.array_equal(rec[2, 3], neg(rec[2, 3 + k])) and sc(2, 3) != sc(2, 3 + k)
    assert np.array_equal(rec[3, 3], neg(rec[3, 3 + k])) and sc(3, 3) == sc(3, 3 + k) != 0
    G0 = M.key_wire(cname, sh.mn)[1][0]
    assert np.array_equal(rec[4, 0], G0) and np.array_equal(rec[5, 0], G0) and sc(5, 0) == S[5][sh.fixed_term_index(2)]
    for i in (6, 7):
        for j in range(8):
            assert np.array_equal(rec[i, 3 + j], M.wire_of_dlog(cname, j + 1))
    assert len({sc(7, 3 + j) for j in range(8)}) == 1 and len({sc(6, 3 + j) for j in range(8)}) == 8
    assert np.array_equal(rec[8, 3], inf) and sc(8, 3) != 0 and b.dlogs[8][sh.var_term_index(3)] == 0
    assert np.array_equal(rec[9, sh.NV - 1], inf) and sc(9, sh.NV - 1) != 0
    assert all(np.array_equal(rec[10, v], rec[10, 0]) for v in range(sh.NV)) and len({sc(10, v) for v in range(sh.NV)}) == 1
    assert all(np.array_equal(rec[11, v], rec[11, 0] if v % 2 == 0 else neg(rec[11, 0])) for v in range(sh.NV))
    assert len({sc(11, v) for v in range(sh.NV)}) == 1


def test_gpu_cases_name_every_geometry_class():
    forms = {}
    for cname, n, m, c, count, mv, form, blocks in M.GPU_CASES:
        forms.setdefault(form, set()).add(cname)
        assert n * (mv or m) <= 256 and (mv == 0 or (mv < m and mv & (mv - 1) == 0))
    assert forms[3] == {"bls12_381", "secp256k1", "ed25519"}
    assert forms[1] == {"bls12_381", "ed25519"} == forms[2]
    assert forms[0] == {"bls12_381", "secp256k1", "ed25519"}
    assert all(count % 128 for _, _, _, _, count, _, form, _ in M.GPU_CASES if form == 0)
    nf258 = {(cname, blocks) for cname, n, m, c, count, mv, form, blocks in M.GPU_CASES if 2 * n * m + 2 == 258}
    # edwards25519 too reaches the left-over steps (two and one block: 2 left-over generators)
    assert nf258 == {(cn, bl) for cn in ("bls12_381", "secp256k1") for bl in (1, 2, 3)} | {("ed25519", 1), ("ed25519", 2)}
    # BLS12-381 at NF = 258, W = 32, two blocks: 2 left-over generators x 2 halves x 32 windows = 128 entries over 256 lanes
    assert M.Shape("bls12_381", 16, 8, 4).W == 32
    parities = {M.Shape("bls12_381", n, m, c).W % 2 for cn, n, m, c, *_ in M.GPU_CASES if cn == "bls12_381"}
    assert parities == {0, 1}


# ---- the hook's usage errors: return codes that write nothing ------------------------------------------------------------
def test_hook_is_bound_but_not_part_of_the_public_header():
    from bulletproofsplus_amd import _lib as L
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "bpp_amd.h")).read()
    for s in ("bpp_debug_verifier_mulvec", "bpp_debug_verifier_mulvec_workspace_bytes"):
        assert hasattr(lib, s) and s not in hdr and s not in L.EXPORTS


def test_hook_usage_errors_write_nothing():
    from bulletproofsplus_amd import _lib as L
    lib = L.lib()
    buf = np.full(256, SENTINEL, dtype=np.uint64)
    pb = buf.ctypes.data_as(ctypes.c_void_p)
    geo = np.full(2, 0x77777777, dtype=np.uint32)
    pg = geo.ctypes.data_as(ctypes.c_void_p)
    # A non-null handle that must never be dereferenced: there is no device here to make a real one.  Every call below
    # with `fake` relies on the hook's order of checks (tu_debug.hip): null pointers, count == 0, count too large and
    # workspace_bytes == 0 are all rejected BEFORE the handle is read (debug_view_shape is the first to read it), and the
    # workspace-size function tests count before the view.  Whoever reorders those checks must keep that, or this test
    # reads address 16.
    fake = ctypes.c_void_p(16)
    assert lib.bpp_debug_verifier_mulvec_workspace_bytes(None, 4, 0) == 0
    assert lib.bpp_debug_verifier_mulvec_workspace_bytes(fake, 1 << 40, 0) == 0
    assert lib.bpp_debug_verifier_mulvec(None, 0, pb, pb, 1, pb, pb, 1 << 20, pb, pg, None) < 0
    assert "null" in lib.bpp_last_error().decode()
    for hole in range(4):   # d_points, d_scalars, d_ok, d_workspace
        args = [pb, pb, 1, pb, pb]
        args[hole if hole < 2 else hole + 1] = None
        assert lib.bpp_debug_verifier_mulvec(fake, 0, *args, 1 << 20, pb, pg, None) < 0
        assert "null" in lib.bpp_last_error().decode()
    assert lib.bpp_debug_verifier_mulvec(None, 0, None, None, 0, None, None, 0, None, None, None) < 0
    assert lib.bpp_debug_verifier_mulvec(fake, 0, pb, pb, 1 << 40, pb, pb, 1 << 20, pb, pg, None) < 0
    assert "count" in lib.bpp_last_error().decode()
    assert lib.bpp_debug_verifier_mulvec(fake, 0, pb, pb, 1, pb, pb, 0, pb, pg, None) < 0   # no workspace at all
    assert "workspace too small" in lib.bpp_last_error().decode()
    assert (buf == SENTINEL).all() and (geo == 0x77777777).all()
