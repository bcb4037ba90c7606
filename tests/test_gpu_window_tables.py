"""-m gpu: the verifier's fixed-generator window tables, entry by entry, as k_tbl_bases, k_tbl_fill and affine_chain
(csrc/kernels.hpp) leave them in device memory -- read back through bpp_debug_verifier_table and held to

    T[f][j][d] = [d 2^(off_j)] F_f      at entry went[j] + d - 1 of generator f

which tests/table_cases.py builds with the CPU oracle alone.  Every comparison is exact; nothing here has a tolerance.  Per
case three things are asserted:
  1. the layout the verifier's shape carries (W, top, per_f, every wc[j], every went[j], glv, hgap) is the restated one, the
     table has NF per_f 2N 4 bytes, and create made the number of k_tbl_fill launches the case names;
  2. the entries through k_points_to_wire are the expected points, infinity given as infinity;
  3. the raw device words are the Montgomery image of the expected coordinates word for word, every coordinate below p --
     the canonical form csrc/ec.hpp xyzz_madd_lazy requires of its affine operand.  (The allocation is not zeroed, so an
     entry the builders never wrote fails both.)

Cases (tests/table_cases.py): whole tables of a (4, 1) verifier, NF = 10, at eight layouts -- every entry of every generator,
except the rows in NARROWED; the curve's smallest layout again over a hashed key; a (4, 4) verifier, whose table is that of
all 34 generators; generators that are the point at infinity, the Edwards identity and a point of order 8; and two tables
that take two launches of k_tbl_fill, at sampled generators either side of the slab boundary.

A generator is checked WHOLE (all per_f entries, expected by the chain of additions) or at the SAMPLE places of its windows
(table_cases.sample_places: first, second and last entries of a run and of the window; expected by scalar multiplication).
"""

import ctypes
import functools
import time
from collections import namedtuple

import numpy as np
import pytest

import mulvec_cases as M
import oracle as O
import table_cases as T
from gpu_util import need_gpu
from verdict_corpus import CID

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "id kind cname n m c slabs")

CASES = [Case("whole-%s-c%d" % t[:2], "whole", t[0], T.WHOLE_NM[0], T.WHOLE_NM[1], t[1], 1) for t in T.WHOLE]
CASES += [Case("hashed-%s-c%d" % (cn, c), "hashed", cn, T.WHOLE_NM[0], T.WHOLE_NM[1], c, 1) for cn, c in sorted(T.SMALLEST.items())]
CASES += [Case("prefix-%s-%dx%d-c%d" % T.PREFIX, "prefix", *T.PREFIX, 1)]
CASES += [Case("infinity-secp256k1-c6", "infinity", "secp256k1", 4, 1, 6, 1),
          Case("torsion-ed25519-c5", "torsion", "ed25519", 4, 1, 5, 1)]
CASES += [Case("slabs-%s-%dx%d-c%d" % t[:4], "slabs", *t[:4], 2) for t in T.SLABS]

# Whole-table rows whose CPU reference takes more than about two seconds when every generator is built by the chain: whole
# windows for generators 0, 1, 2 and NF - 1, the sample places for the rest.  None is narrowed: the largest row (ed25519,
# window_bits 8: 39 840 Edwards additions) was measured at 1.6 s, every other one below 1.5 s.
NARROWED = set()
INF_G1, TORSION_H0 = 2 + 1, 2 + 4 + 0       # table numbering at (4, 1): g, h, G_0..G_3, H_0..H_3
MAXW = 128                                   # csrc/kernels.hpp VS_MAXW: out_layout never holds more windows


@functools.lru_cache(maxsize=None)
def _whole(cname, c, F, by_additions=False):
    """the reference of one generator's whole table, computed once and shared by the cases over the same key"""
    return T.generator_table(cname, T.layout(cname, c), F, by_additions)


def _spans(L, wins):
    """the sample places of the given windows as (first entry, [(j, d), ..]) runs of neighbouring entries"""
    out = []
    for j in wins:
        run = []
        for d in T.sample_places(L.entries[j]):
            if run and run[-1][1] + 1 != d:
                out.append((L.went[j] + run[0][1] - 1, run))
                run = []
            run.append((j, d))
        out.append((L.went[j] + run[0][1] - 1, run))
    return out


class Table:
    """one case: the verifier, what the hook reported, and per checked span (f, first, places, raw, wire, expected)"""


def _read(lib, bv, f, first, count, N, PW):
    from bulletproofsplus_amd import _lib
    raw = np.full((count, 2 * N), 0xA5A5A5A5, dtype=np.uint32)
    wire = np.full((count, PW), 0x7777777777777777, dtype=np.uint64)
    _lib.check(lib.bpp_debug_verifier_table(bv.handle, f, first, count, raw.ctypes.data_as(ctypes.c_void_p),
                                            wire.ctypes.data_as(ctypes.c_void_p), None), "bpp_debug_verifier_table")
    return raw, wire


@pytest.fixture(scope="module", params=CASES, ids=lambda c: c.id)
def table(request):
    """builds the case's verifier, reads the checked entries back and computes their reference; the verifier is destroyed
    before the next case builds its own"""
    need_gpu()
    import bulletproofsplus_amd as B
    from bulletproofsplus_amd import _lib
    lib = _lib.lib()
    case = request.param
    cname, n, m, c = case.cname, case.n, case.m, case.c
    cid, mn = CID[cname], n * m
    NF = 2 * mn + 2
    L = T.layout(cname, c)
    f_ = T.base_field(cname)
    N, PW = f_.N, O.point_words(cid)
    a = B.Arith.init(cname)

    # ---- the key, and the plan: which generators are checked whole, which at the sample places of which windows ----
    t0 = time.perf_counter()
    by_additions = set()
    wins = range(L.W)
    if case.kind == "hashed":
        pk = B.PublicKey.hashed(a, mn, b"window tables")
        F = O.wire_to_points(cid, np.concatenate([pk.gh, pk.G_vec, pk.H_vec]))
        assert len(set(F)) == NF and None not in F
    elif case.kind == "slabs":
        pk = B.PublicKey.new(a, mn)
        kw = np.concatenate([pk.gh, pk.G_vec, pk.H_vec])
        gens, wins = T.slab_samples(L, NF)
        dl = M.Shape(cname, n, m, c).fixed_dlogs()
        F = {f: O.wire_to_point(cid, M.wire_of_dlog(cname, dl[f])) for f in gens}
        for f in gens:                                   # the reference's generators, at the places looked at
            assert np.array_equal(kw[f], O.point_to_wire(cid, F[f])), f
    else:
        F = T.key_points(cname, mn)
        if case.kind == "infinity":
            F[INF_G1] = None
        if case.kind == "torsion":
            F[INF_G1], F[TORSION_H0] = None, T.order8_point()
            by_additions.add(TORSION_H0)
        kw = O.points_to_wire(cid, F)
        if case.kind in ("infinity", "torsion"):
            pk = B.PublicKey.from_points(a, kw[:2], kw[2:2 + mn], kw[2 + mn:])
        else:
            pk = B.PublicKey.new(a, mn)                  # the reference's generators
            assert np.array_equal(np.concatenate([pk.gh, pk.G_vec, pk.H_vec]), kw)
    if case.kind == "slabs":
        whole, sampled = [], gens
    elif case.kind == "prefix":
        whole = list(T.PREFIX_WHOLE)
        sampled = [f for f in range(NF) if f not in whole]
    elif (cname, c) in NARROWED:
        whole = [0, 1, 2, NF - 1]
        sampled = [f for f in range(NF) if f not in whole]
    else:
        whole, sampled = list(range(NF)), []
    t_key = time.perf_counter() - t0

    # ---- the device: build, read back ----
    t0 = time.perf_counter()
    bv = B.BatchVerifier(pk, n, m, window_bits=c)
    t_build = time.perf_counter() - t0
    tb = Table()
    tb.case, tb.L, tb.NF, tb.N, tb.bv, tb.lib = case, L, NF, N, bv, lib
    try:
        lay = np.full(7 + 2 * MAXW, 0x5A5A5A5A, dtype=np.uint32)
        _lib.check(lib.bpp_debug_verifier_table(bv.handle, 0, 0, 0, None, None, lay.ctypes.data_as(ctypes.c_void_p)),
                   "bpp_debug_verifier_table")
        tb.layout_words = lay
        tb.table_bytes = lib.bpp_verifier_table_bytes(bv.handle)
        spans = [(f, 0, None) for f in whole]
        spans += [(f, first, places) for f in sampled for first, places in _spans(L, wins)]
        read = []
        for f, first, places in spans:
            count = L.per_f if places is None else len(places)
            read.append(_read(lib, bv, f, first, count, N, PW))
        t_gpu = time.perf_counter() - t0

        # ---- the reference ----
        t0 = time.perf_counter()
        tb.spans = []
        for (f, first, places), (raw, wire) in zip(spans, read):
            if places is None:
                want = _whole(cname, c, F[f], f in by_additions)
            else:
                want = [T.entry(cname, L, F[f], j, d) for j, d in places]
            tb.spans.append((f, first, places, raw, wire, want))
        t_cpu = time.perf_counter() - t0
        tb.entries = sum(len(s[5]) for s in tb.spans)
        print("\nwindow tables %s: NF %d per_f %d table %.3f GB, %d entries checked (%d generators whole, %d sampled); "
              "create %.2f s, create and read-back %.2f s, CPU reference %.2f s (key %.2f s)"
              % (case.id, NF, L.per_f, tb.table_bytes / 1e9, tb.entries, len(whole), len(sampled), t_build, t_gpu, t_cpu, t_key))
        yield tb
    finally:
        bv.close()


def _where(tb, f, first, places, i):
    if places is not None:
        return "generator %d window %d d %d" % ((f,) + places[i])
    e = first + i
    j = max(j for j in range(tb.L.W) if tb.L.went[j] <= e)
    return "generator %d window %d d %d" % (f, j, e - tb.L.went[j] + 1)


def test_layout_is_the_restated_one(table):
    tb, L = table, table.L
    want = T.layout_words(L, 0, tb.case.slabs)
    got = tb.layout_words[:len(want)].tolist()
    names = ["W", "top", "per_f", "glv", "hgap", "slabs", "runs_per_generator"]
    for name, g, w in zip(names, got, want):
        assert g == w, "%s: the verifier carries %d, the restated layout %d" % (name, g, w)
    assert got[7:7 + L.W] == list(L.widths), "wc[]"
    assert got[7 + L.W:] == list(L.went), "went[]"
    assert (tb.layout_words[len(want):] == 0x5A5A5A5A).all()        # nothing written past went[W - 1]
    assert tb.table_bytes == tb.NF * L.per_f * 2 * tb.N * 4
    if tb.case.kind == "slabs":
        assert tb.NF > T.slab_generators(L)
        assert tb.table_bytes > 4 * 10**9


def test_entries_on_the_wire_are_the_multiples(table):
    tb = table
    cid = CID[tb.case.cname]
    assert tb.entries > 0
    for f, first, places, raw, wire, want in tb.spans:
        got = O.wire_to_points(cid, wire)
        if got != want:
            bad = [i for i in range(len(want)) if got[i] != want[i]]
            raise AssertionError("%s: %d of %d entries differ, first at %s: got %s, want %s" % (
                tb.case.id, len(bad), len(want), _where(tb, f, first, places, bad[0]), got[bad[0]], want[bad[0]]))
    if tb.case.kind == "infinity":
        assert all(w is None for f, _, _, _, _, want in tb.spans if f == INF_G1 for w in want)
        assert all(int(wire[i, -1]) == 1 for f, _, _, _, wire, _ in tb.spans if f == INF_G1 for i in range(len(wire)))
    if tb.case.kind == "torsion":
        for f, _, _, _, _, want in tb.spans:
            if f == INF_G1:
                assert want == [None] * tb.L.per_f
            if f == TORSION_H0:                          # the 8-torsion in window 0, the identity from off_j >= 3 on
                assert want[7] is None and None not in want[:7] and want[8:15] == want[:7]
                assert tb.L.offs[1] >= 3 and want[tb.L.went[1]:] == [None] * (tb.L.per_f - tb.L.went[1])


def test_raw_words_are_the_canonical_montgomery_image(table):
    tb = table
    cname = tb.case.cname
    p = T.base_field(cname).p
    for f, first, places, raw, wire, want in tb.spans:
        exp = T.raw_image(cname, want)
        if not np.array_equal(raw, exp):
            bad = np.flatnonzero((raw != exp).any(axis=1))
            i = int(bad[0])
            raise AssertionError("%s: %d of %d raw entries differ, first at %s: got %s, want %s" % (
                tb.case.id, len(bad), len(want), _where(tb, f, first, places, i), raw[i].tolist(), exp[i].tolist()))
        for i, (x, y) in enumerate(T.raw_coordinates(cname, raw)):
            assert x < p and y < p, "a coordinate in [p, 2p) at %s" % _where(tb, f, first, places, i)
    if tb.case.kind == "infinity":
        assert all(not raw.any() for f, _, _, raw, _, _ in tb.spans if f == INF_G1)


def test_hook_refuses_what_lies_outside_the_table():
    """usage errors are return codes before any launch, and write nothing; count = 0 is a no-op"""
    need_gpu()
    import bulletproofsplus_amd as B
    from bulletproofsplus_amd import _lib
    lib = _lib.lib()
    a = B.Arith.init("secp256k1")
    bv = B.BatchVerifier(B.PublicKey.new(a, 4), 4, 1, window_bits=3)
    try:
        L = T.layout("secp256k1", 3)
        raw = np.full((4, 16), 0xA5A5A5A5, dtype=np.uint32)
        wire = np.full((4, 9), 0x7777777777777777, dtype=np.uint64)
        lay = np.full(7 + 2 * MAXW, 0x5A5A5A5A, dtype=np.uint32)
        ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        hook = lambda f, first, count: lib.bpp_debug_verifier_table(bv.handle, f, first, count, ptr(raw), ptr(wire), ptr(lay))
        for args in ((10, 0, 1), (0xFFFFFFFF, 0, 1), (0, L.per_f, 1), (0, L.per_f - 3, 4), (0, 0xFFFFFFFF, 2), (0, 2, 0xFFFFFFFF),
                     (0, L.per_f + 1, 0)):
            assert hook(*args) < 0, args
            assert "beyond" in lib.bpp_last_error().decode()
        assert lib.bpp_debug_verifier_table(None, 0, 0, 1, ptr(raw), ptr(wire), ptr(lay)) < 0
        assert (raw == 0xA5A5A5A5).all() and (wire == 0x7777777777777777).all() and (lay == 0x5A5A5A5A).all()
        assert hook(9, L.per_f, 0) == 0 and hook(0, 0, 0) == 0               # nothing to read: the layout alone
        assert (raw == 0xA5A5A5A5).all() and (wire == 0x7777777777777777).all() and lay[0] == L.W
        assert hook(9, L.per_f - 4, 4) == 0                                   # the last entries of the last generator
        assert not (raw == 0xA5A5A5A5).all(axis=1).any() and not (wire == 0x7777777777777777).all(axis=1).any()
        r2, w2 = _read(lib, bv, 9, L.per_f - 4, 4, 8, 9)
        assert np.array_equal(r2, raw) and np.array_equal(w2, wire)
        # either output alone
        assert lib.bpp_debug_verifier_table(bv.handle, 9, L.per_f - 4, 4, None, ptr(w2), None) == 0
        assert lib.bpp_debug_verifier_table(bv.handle, 9, L.per_f - 4, 4, ptr(r2), None, None) == 0
        assert np.array_equal(r2, raw) and np.array_equal(w2, wire)
    finally:
        bv.close()
