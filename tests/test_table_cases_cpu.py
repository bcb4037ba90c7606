"""CPU: the case builder of the window-table tests (tests/table_cases.py) is itself right.

  * The layout figures the GPU cases name (W, entries of the signed windows, top, per_f; for the several-slab cases also the
    runs per generator, the generators per slab and NF) come out of the restated formulas.
  * The recoding ties the extents to the readers: whatever value the recoding can be handed, every signed digit stays within
    the entries its window has, every top digit within `top`, and the largest value reaches `top` exactly -- a table with one
    entry fewer would be read past its end, one with more holds entries nobody reads.
  * The chain of additions that builds the expected windows lands on the scalar multiples [d 2^(off_j)] F at every sample
    place of every window, and the raw image is the Montgomery form of the coordinates.
No GPU needed: nothing here reaches a device."""

import random

import numpy as np
import pytest

import mulvec_cases as M
import pyref as P
import table_cases as T

LAYOUTS = sorted({(c[0], c[1]) for c in T.WHOLE} | {(T.PREFIX[0], T.PREFIX[3])} | {(c[0], c[3]) for c in T.SLABS})


def _lid(t):
    return "%s-c%d" % t


@pytest.mark.parametrize("case", T.WHOLE, ids=lambda t: "%s-c%d" % t[:2])
def test_whole_table_figures_come_out_of_the_restatement(case):
    cname, c, W, signed, top, per_f = case
    L = T.layout(cname, c)
    assert (L.W, L.top, L.per_f) == (W, top, per_f)
    assert tuple(sorted(set(L.entries[:-1]))) == signed
    assert L.entries[-1] == top and L.widths[-1] == 0 and len(L.widths) == len(L.went) == len(L.offs) == W
    assert L.went[0] == 0 and all(L.went[j + 1] == L.went[j] + L.entries[j] for j in range(W - 1))
    assert L.offs[0] == 0 and all(L.offs[j + 1] == L.offs[j] + L.widths[j] for j in range(W - 1))
    assert L.runs == sum(-(-e // 32) for e in L.entries) and T.slab_generators(L) >= 10      # one slab
    NF = 2 * T.WHOLE_NM[0] * T.WHOLE_NM[1] + 2
    assert NF == 10
    if not L.glv:
        assert L.W == (P.CURVES[cname]["r"].bit_length() - 1) // c + 1 and set(L.widths[:-1]) == {c}
    else:
        assert list(L.widths[:-1]) == sorted(L.widths[:-1])          # the wider windows on top


def test_smallest_rows_and_the_prefix_case_are_rows_of_the_table():
    for cname, c in T.SMALLEST.items():
        assert c == min(t[1] for t in T.WHOLE if t[0] == cname)
    cname, n, m, c = T.PREFIX
    assert 2 * n * m + 2 == 34 == max(T.PREFIX_WHOLE) + 1 and (cname, c) in {t[:2] for t in T.WHOLE}
    assert T.slab_generators(T.layout(cname, c)) >= 34


@pytest.mark.parametrize("case", T.SLABS, ids=lambda t: "%s-c%d" % (t[0], t[3]))
def test_slab_figures_come_out_of_the_restatement(case):
    cname, n, m, c, W, top, per_f, runs, s, NF = case
    L = T.layout(cname, c)
    assert (L.W, L.top, L.per_f, L.runs) == (W, top, per_f, runs)
    assert T.slab_generators(L) == s == (1 << 21) // runs and 2 * n * m + 2 == NF
    assert s < NF <= 2 * s                                           # two launches of k_tbl_fill, no more
    gens, wins = T.slab_samples(L, NF)
    assert gens == [0, 1, s - 1, s, s + 1, NF - 1]
    if cname == "bls12_381":
        assert sorted(set(L.widths[:-1])) == [12, 13]
        t = L.widths.index(13)
        assert wins == sorted({0, 1, t - 1, t, W - 2, W - 1}) and L.widths[t - 1] == 12
    else:
        assert wins == [0, 1, W - 2, W - 1]


@pytest.mark.parametrize("lay", LAYOUTS, ids=_lid)
def test_recoding_stays_inside_the_table_and_reaches_its_last_entry(lay):
    cname, c = lay
    L = T.layout(cname, c)
    vmax = T.max_value(cname)
    rng = random.Random("table extents %s %d" % lay)
    vals = [0, 1, vmax] + [rng.randrange(vmax + 1) for _ in range(300)]
    if not L.glv:
        assert vmax == P.CURVES[cname]["r"] - 1
    else:
        assert vmax == M.HALF_MAX
    for v in vals:
        d = T.recode(L, v)
        assert len(d) == L.W
        assert sum(x << o for x, o in zip(d, L.offs)) == v                    # the digits say the value
        for j in range(L.W - 1):
            assert abs(d[j]) <= 1 << (L.widths[j] - 1) == L.entries[j], (v, j)
        assert 0 <= d[-1] <= L.top, v
    assert T.recode(L, vmax)[-1] == L.top                                   # the last entry of the top window is read
    # ... and the last one of every signed window, which only the most negative digit -2^(c_j - 1) selects
    vlow = (1 << L.offs[-1]) - sum(e << o for e, o in zip(L.entries[:-1], L.offs))
    assert 0 <= vlow <= vmax and T.recode(L, vlow) == [-e for e in L.entries[:-1]] + [1]


def test_sample_places():
    assert T.sample_places(2) == [1, 2]
    assert T.sample_places(4) == [1, 2, 3, 4]
    assert T.sample_places(16) == [1, 2, 3, 15, 16]
    assert T.sample_places(32) == [1, 2, 3, 31, 32]
    assert T.sample_places(43) == [1, 2, 3, 31, 32, 33, 34, 42, 43]
    assert T.sample_places(65536) == [1, 2, 3, 31, 32, 33, 34, 63, 64, 65, 65535, 65536]


@pytest.mark.parametrize("cname", sorted(T.SMALLEST))
def test_chain_of_additions_lands_on_the_scalar_multiples(cname):
    """one generator at the curve's smallest whole-table case: every sample place of every window"""
    L = T.layout(cname, T.SMALLEST[cname])
    F = T.key_points(cname, 4)[7]                     # H_1 = 10 g
    tab = T.generator_table(cname, L, F)
    for j in range(L.W):
        for d in T.sample_places(L.entries[j]):
            assert tab[L.went[j] + d - 1] == T.entry(cname, L, F, j, d), (j, d)
            assert tab[L.went[j] + d - 1] is not None
    # the additions-only construction (used for a point outside the prime-order subgroup) is the same table
    if cname == "ed25519":
        assert T.generator_table(cname, L, F, by_additions=True) == tab
    assert T.generator_table(cname, L, None) == [None] * L.per_f


def test_raw_image_is_the_montgomery_form():
    for cname in sorted(T.SMALLEST):
        f = T.base_field(cname)
        pts = T.key_points(cname, 4)[:3] + [None]
        raw = T.raw_image(cname, pts)
        assert raw.shape == (4, 2 * f.N) and raw.dtype == np.uint32
        Rinv = pow(f.R, -1, f.p)
        co = T.raw_coordinates(cname, raw)
        for pt, (x, y) in zip(pts[:3], co):
            assert x < f.p and y < f.p and (x * Rinv % f.p, y * Rinv % f.p) == pt
        if cname == "ed25519":
            assert co[3] == (0, f.R % f.p)
        else:
            assert co[3] == (0, 0) and not raw[3].any()


def test_order8_point_cycles_through_the_torsion():
    G = P.EdwardsGroup(P.CURVES["ed25519"])
    Tt = T.order8_point()
    mult = T.chain("ed25519", Tt, 16)
    assert mult[7] is None and mult[15] is None and None not in mult[:7]
    assert len(set(mult[:7])) == 7 and mult[8:15] == mult[:7]
    L = T.layout("ed25519", 5)
    w1 = T.window_by_additions("ed25519", L, Tt, 1)              # off 5: every multiple of 32 T is the identity
    assert w1 == [None] * 16
    assert T.window_by_additions("ed25519", L, Tt, 0) == mult
    assert G.on_curve(Tt)
