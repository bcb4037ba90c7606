"""The adversarial corpus (tests/verdict_corpus.py) means what its case names say -- checked on the host against the
C oracle and the big-integer restatement, no device needed.  tests/test_gpu_verdict_parity.py feeds it to every
verify entry point of the engine."""

import numpy as np
import pytest

import oracle as O
import pyref as P
import verdict_corpus as VC

SHAPES = [(c, s) for c in ("bls12_381", "secp256k1", "ed25519") for s in VC.SHAPES]


@pytest.mark.parametrize("cname,shape", SHAPES)
def test_corpus_cases_are_what_they_say(cname, shape):
    cp = VC.corpus(cname, *shape)
    grp, L = cp.grp, cp.L
    base = cp.by_name("valid_1")
    names = [c.name for c in cp.cases]
    assert len(set(names)) == len(names)
    for nm in ("valid_1", "valid_2", "v_zero", "v_max", "gamma_zero", "gamma_rm1", "v_wrap40"):
        assert cp.by_name(nm).expect == 0, nm
    assert not np.array_equal(cp.by_name("valid_1").pts, cp.by_name("valid_2").pts)
    for nm in ("v_2n", "v_wrap31", "flip_r", "flip_s", "flip_d", "wrong_k", "off_curve_wA"):
        assert cp.by_name(nm).expect == 1, nm
    for c in cp.cases:
        if c.name.startswith("move_") or c.name == "neg_Vlast":      # the point really moved
            assert not (np.array_equal(c.pts, base.pts) and np.array_equal(c.V, base.V)), c.name
            assert c.expect == 1, c.name
        if c.enc_ok and c.k_ok:
            for w in list(c.pts) + list(c.V):
                assert w[2 * L] or grp.on_curve(O.wire_to_point(cp.cid, w)), c.name
        if c.name.startswith("nc_"):
            # non-canonical scalar: the definition is the reduced value, and the C oracle given the raw words agrees
            raw = O.limbs_to_int(c.sc[0])
            assert raw >= cp.r and raw < (1 << 256) and raw % cp.r == O.limbs_to_int(base.sc[0])
            assert c.expect == base.expect == 0 and c.status == 2
            if cname != "ed25519":
                assert O.range_verify(cp.opk, cp.n, cp.m, c.pts, c.sc, c.V) == 0
        if c.status is not None:     # the container status: pyref's decoder on pyref's encoding
            blob, _ = VC.encode_case(cp, c)
            dec = P.decode_proof(cp.curve, grp, cp.n, cp.m, blob)
            assert (dec is None) == (c.status == 2), c.name
    off = cp.by_name("off_curve_wA")
    assert not grp.on_curve(O.wire_to_point(cp.cid, off.pts[1]))
    if cname != "ed25519":
        assert O.range_verify(cp.opk, cp.n, cp.m, cp.by_name("wrong_k").pts, base.sc, base.V) == 1
        # the non-canonical infinity is judged as the canonical one
        c5 = cp.by_name("L0_inf_flag5")
        assert c5.pts[3, 2 * L] == 5 and O.range_verify(cp.opk, cp.n, cp.m, VC.canonical_inf(cp, c5.pts), c5.sc, c5.V) == c5.expect
    if "L0_x_plus_p" in names:
        x = O.limbs_to_int(cp.by_name("L0_x_plus_p").pts[3, :L])
        assert x >= cp.p and x - cp.p == O.limbs_to_int(base.pts[3, :L])
    if cname == "ed25519":
        assert any(c.name.startswith("nc_r_plus_1") for c in cp.cases)   # j = 14 or 15: past the old 4-round host loop


@pytest.mark.parametrize("shape", VC.SHAPES)
def test_bls_out_of_g1_cases(shape):
    cp = VC.corpus("bls12_381", *shape)
    grp = cp.grp
    T = VC.bls_T()
    assert grp.on_curve(T) and not P.point_in_prime_subgroup(cp.curve, grp, T)
    base = cp.by_name("valid_1")
    for nm in ("R0_plus_T", "A_eq_T", "cancel_pair"):
        c = cp.by_name(nm)
        moved = [i for i in range(c.pts.shape[0]) if not np.array_equal(c.pts[i], base.pts[i])]
        assert moved and c.shifted and c.status == 2
        for i in moved:
            Pt = O.wire_to_point(0, c.pts[i])
            assert O.on_curve(0, c.pts[i]) and not P.point_in_prime_subgroup(cp.curve, grp, Pt), (nm, i)
    assert cp.by_name("R0_plus_T").expect == 1 and cp.by_name("A_eq_T").expect == 1
    # the cancelling pair: the full-curve sum is unchanged (accept), either shift alone is rejected
    c = cp.by_name("cancel_pair")
    i, j, k3 = c.pair
    s = base.mv_scalars
    assert (s[cp.scalar_index(i)] + k3 * s[cp.scalar_index(j)]) % 3 == 0
    assert c.expect == 0
    for drop in (i, j):
        one = c.pts.copy()
        one[drop] = base.pts[drop]
        assert O.range_verify(cp.opk, cp.n, cp.m, one, base.sc, base.V) == 1


@pytest.mark.parametrize("shape", VC.SHAPES)
def test_ed25519_torsion_cases(shape):
    cp = VC.corpus("ed25519", *shape)
    grp = cp.grp
    T4, T8 = VC.ed_torsion(4), VC.ed_torsion(8)
    assert grp.is_zero(grp.mul(T4, 4)) and not grp.is_zero(grp.mul(T4, 2))
    assert grp.is_zero(grp.mul(T8, 8)) and not grp.is_zero(grp.mul(T8, 4))
    base = cp.by_name("valid_1")
    assert cp.by_name("A_plus_T4").expect == base.expect == 0
    names = [c.name for c in cp.cases]
    assert "T8_odd" in names
    for c in cp.cases:
        if c.t8:
            s = base.mv_scalars[cp.scalar_index(c.moved_idx)]
            assert (s % 2 == 0) == (c.name == "T8_even")
            # the class the name says: the sum moves by s T8, inside E[4] iff s is even
            assert grp.is_identity_class(c.result) == (s % 2 == 0) and c.expect == s % 2
    # the fast group law of the corpus is pyref's: one case checked end to end with pyref's own verify
    pk = P.PublicKey(P.EdwardsGroup(cp.curve), cp.mn)
    pp = O.wire_to_points(2, base.pts)
    k = cp.k
    pf = P.RangeProof(pp[0], P.WeightedInnerProductProof(pp[3:3 + k], pp[3 + k:3 + 2 * k], pp[1], pp[2],
                                                        *O.wire_to_scalars(base.sc)))
    assert pf.verify(pk, cp.n, O.wire_to_points(2, base.V)) is True


@pytest.mark.parametrize("cname", ["bls12_381", "secp256k1"])
def test_transcript_variants(cname):
    cp = VC.corpus(cname, 8, 2, transcript=True)
    exp = {c.name: c.expect for c in cp.cases}
    want = {"valid_1": 0, "valid_2": 0, "flip_r": 1, "flip_s": 1, "flip_d": 1, "nc_r_plus_r": 0}
    if cname == "secp256k1":        # r > 2^255: r' + r does not fit in 256 bits
        del want["nc_r_plus_r"]
    assert exp == want
    fixed = VC.corpus(cname, 8, 2)
    assert not np.array_equal(cp.by_name("valid_1").pts, fixed.by_name("valid_1").pts)   # other challenges, other proof
    # the fixed-challenge verifier rejects the transcript proof
    c = cp.by_name("valid_1")
    assert O.range_verify(fixed.opk, 8, 2, c.pts, c.sc, c.V) == 1
