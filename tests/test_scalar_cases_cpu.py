"""The scalar-stage case builder (tests/scalar_cases.py) against itself and against the C oracle, on the CPU: the two
restatements of the verifier's MulVec scalars agree on every non-zero row at every shape the GPU sweep runs, both equal the
oracle's RangeProof::verify at the reference's literals, words >= r stand for their residues, and a zeroed challenge changes
exactly the outputs the closed forms say it enters (so the inv0 convention of the direct restatement is pinned, not
vacuous)."""

import random

import numpy as np
import pytest

import oracle as O
import pyref as P
import scalar_cases as S

# every shape of tests/test_gpu_verifier_scalars.py: the verifiers' own shapes and their prefix views
SWEEP_SHAPES = [(1, 1), (1, 2), (1, 32), (1, 64), (2, 1), (2, 2), (2, 32), (2, 64), (4, 1), (4, 4), (4, 8), (8, 1), (8, 2),
                (8, 4), (8, 8), (8, 16), (64, 1)]
BLS_ONLY_SHAPES = [(64, 2), (64, 4), (64, 16), (64, 32), (32, 64), (64, 64)]
SEAM_SHAPES = [(4, 0), (4, 3), (64, 1), (128, 3), (512, 0), (512, 64)]


def _shapes():
    out = [(c, n, m) for c in S.CURVES for n, m in SWEEP_SHAPES]
    return out + [("bls12_381", n, m) for n, m in BLS_ONLY_SHAPES]


@pytest.mark.parametrize("curve,n,m", _shapes(), ids=lambda v: str(v))
def test_the_two_restatements_agree_on_every_non_zero_row(curve, n, m):
    k = S.log2(n * m)
    names = S.row_names(k)
    assert {"one_hot(%d)" % t for t in range(k)} <= set(names)
    big = n * m >= 2048                        # one pass over the rows there, two (fresh values) elsewhere
    rows = S.rows(curve, n, m, len(names) * (1 if big else 2), 1)
    assert [r.name for r in rows[:len(names)]] == names
    for row in rows:
        a, b = S.range_scalars(curve, n, m, *row.args()), S.range_scalars_direct(curve, n, m, *row.args())
        assert len(a) == len(b) == S.n_scalars(n, m)
        bad = [i for i in range(len(a)) if a[i] != b[i]]
        assert not bad, (row.name, bad[:8])


@pytest.mark.parametrize("curve", S.CURVES)
@pytest.mark.parametrize("length,nv", SEAM_SHAPES)
def test_the_two_seam_restatements_agree(curve, length, nv):
    k = S.log2(length)
    names = [x for x in S.seam_row_names(k) if not x.startswith("zero")]
    for row in S.seam_rows(curve, length, nv, len(names), 2, names):
        a, b = S.seam_scalars(curve, length, *row.args()), S.seam_scalars_direct(curve, length, *row.args())
        assert len(a) == len(b) == 2 * length + 2 * k + 5 + nv
        bad = [i for i in range(len(a)) if a[i] != b[i]]
        assert not bad, (row.name, bad[:8])


@pytest.mark.parametrize("cname,n,values", [("bls12_381", 8, [200]), ("bls12_381", 4, [3, 12]), ("secp256k1", 8, [77]),
                                            ("secp256k1", 2, [1, 2, 3, 0])])
def test_both_equal_the_c_oracle_at_the_literals(cname, n, values):
    cid, m = O.CURVE_IDS[cname], len(values)
    k = S.log2(n * m)
    opk = O.PublicKey(cid, n * m)
    pts, sc, V = O.range_prove(opk, n, values, [5 + 3 * j for j in range(m)])
    rc, exp, _ = O.range_verify(opk, n, m, pts, sc, V, want_scalars=True, skip_msm=True)
    assert rc == 0
    T = P.Transcript
    y, z = (T.Y_SINGLE, T.Z_SINGLE) if m == 1 else (T.Y_MULTI, T.Z_MULTI)
    args = (y, z, T.E_FINAL, [T.E_ROUND] * k, O.wire_to_scalars(sc))
    assert (y, z, T.E_FINAL, T.E_ROUND) == ((7, 7) if m == 1 else (12, 23)) + (99, 7)
    want = O.wire_to_scalars(exp)
    assert S.range_scalars(cname, n, m, *args) == want
    assert S.range_scalars_direct(cname, n, m, *args) == want
    assert np.array_equal(S.to_wire(want), exp)


def test_the_literals_are_restored():
    T = P.Transcript
    before = tuple(getattr(T, a) for a in S._Literals.NAMES)
    row = S.rows("secp256k1", 2, 2, 1, 3, ["zero_y"])[0]
    with pytest.raises(ValueError):             # pyref has no inverse of 0 -- and must still put the literals back
        S.range_scalars("secp256k1", 2, 2, *row.args())
    assert tuple(getattr(T, a) for a in S._Literals.NAMES) == before == (7, 7, 12, 23, 99, 7)


@pytest.mark.parametrize("curve", S.CURVES)
def test_lifts_are_the_patterns_of_a_residue(curve):
    r = S.order(curve)
    per_curve = {"bls12_381": (2, 1), "secp256k1": (1, 0), "ed25519": (15, 14)}[curve]   # lifts of 0, of r - 1
    assert (len(S.lifts(curve, 0)), len(S.lifts(curve, r - 1))) == per_curve
    for x in (0, 1, S.liftable(curve) - 1, S.TOP % r):
        ls = S.lifts(curve, x)
        assert ls and all(r <= v < 1 << 256 and v % r == x for v in ls) and ls[-1] + r >= 1 << 256
        assert S.lift(curve, x) == ls[-1]
    assert S.lift(curve, S.TOP % r) == S.TOP
    assert S.to_wire([S.TOP]).tolist() == [[0xFFFFFFFFFFFFFFFF] * 4]


@pytest.mark.parametrize("curve", S.CURVES)
@pytest.mark.parametrize("n,m", [(8, 2), (64, 1), (8, 16), (1, 1)])
def test_lifted_rows_give_the_scalars_of_their_residues(curve, n, m):
    r = S.order(curve)
    k = S.log2(n * m)
    for row in S.rows(curve, n, m, 3, 4, ["lifted"]):
        given = [row.y, row.e, row.s3[0]] + ([row.e_rounds[k // 2]] if k else [])
        assert all(r <= v < 1 << 256 for v in given) and row.z == S.TOP
        res = row.residues(r)
        assert all(0 < v < r for v in res.challenges())
        want = S.range_scalars_direct(curve, n, m, *res.args())
        assert S.range_scalars_direct(curve, n, m, *row.args()) == want
        assert S.range_scalars(curve, n, m, *row.args()) == want
    stm_row = S.seam_rows(curve, 8, 2, 1, 4, ["lifted"])[0]
    lifted_stm = [x + r if x < S.liftable(curve) else x for x in stm_row.stm]
    want = S.seam_scalars_direct(curve, 8, *stm_row.args())
    assert S.seam_scalars_direct(curve, 8, stm_row.y % r, lifted_stm, stm_row.e % r, stm_row.e_rounds, stm_row.s3) == want


@pytest.mark.parametrize("curve", S.CURVES)
@pytest.mark.parametrize("n,m", [(8, 2), (64, 1), (8, 16)])
def test_a_zeroed_challenge_changes_exactly_the_outputs_it_enters(curve, n, m):
    """zero row vs the same row with the zero replaced by a non-zero value: equal on independent_outputs -- the leading 1,
    and (y) the head, h_exp, L, R; (e, m > 1) L, R, V; (e, m = 1) h_exp; (round t) head, g_exp, h_exp, V and the L, R of the
    other rounds -- and different everywhere else.  The lifted zero is the zero."""
    r = S.order(curve)
    k = S.log2(n * m)
    rng = random.Random(5)
    names = S.zero_row_names(k)
    assert len(names) == 8
    for row in S.rows(curve, n, m, len(names), 5, names):
        what = S.zeroed(row.name)
        z0 = S.range_scalars_direct(curve, n, m, *row.args())
        if "lifted" in row.name:
            given = row.y if what == "y" else row.e if what == "e" else row.e_rounds[what]
            assert given >= r and given % r == 0
            assert z0 == S.range_scalars_direct(curve, n, m, *S.healed(row, 0).args())
        keep = set(S.independent_outputs(n, m, what))
        for value in (1, r - 1, rng.randrange(2, r)):
            h = S.range_scalars_direct(curve, n, m, *S.healed(row, value).args())
            assert h == S.range_scalars(curve, n, m, *S.healed(row, value).args())
            same = {i for i in range(len(z0)) if z0[i] == h[i]}
            assert same == keep, (row.name, value, sorted(same ^ keep)[:8])
        # the zero itself: inv0 leaves 0 where the inverse would stand
        if what == "e" and m > 1:
            assert z0[1] == z0[2] == 0
        if what not in ("y", "e"):
            assert z0[5 + what] == 0 and z0[5 + k + what] == 0


@pytest.mark.parametrize("curve", S.CURVES)
def test_a_zeroed_seam_challenge_changes_exactly_the_outputs_it_enters(curve):
    length, nv = 16, 2
    r = S.order(curve)
    k = S.log2(length)
    names = ["zero_e", "zero_round(0)", "zero_round(%d)" % (k - 1), "zero_y"]
    for row in S.seam_rows(curve, length, nv, len(names), 6, names):
        what = S.zeroed(row.name)
        z0 = S.seam_scalars_direct(curve, length, *row.args())
        keep = set(S.independent_outputs(length, nv, what, seam=True)) if nv else None
        for value in (1, r - 1, 12345):
            if what == "y":
                h = S.seam_scalars_direct(curve, length, value, row.stm, row.e, row.e_rounds, row.s3)
            elif what == "e":
                h = S.seam_scalars_direct(curve, length, row.y, row.stm, value, row.e_rounds, row.s3)
            else:
                er = list(row.e_rounds)
                er[what] = value
                h = S.seam_scalars_direct(curve, length, row.y, row.stm, row.e, er, row.s3)
            same = {i for i in range(len(z0)) if z0[i] == h[i]}
            assert same == keep, (row.name, value, sorted(same ^ keep)[:8])
