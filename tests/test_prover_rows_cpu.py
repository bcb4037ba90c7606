"""The prover's rows (tests/prover_rows.py) held against each other without a GPU: the reference's direction (model A) equals
the closed forms of csrc/prover_batch.hpp (model B) on every row at every k; every named fault of model B changes an output
somewhere in the corpus at every k where it can; model A's delta' is recover_rows' forward delta'; and with the literals
model A is pyref's shadow prover, points included (the shadow group is the group of discrete logs)."""

import pytest

import prover_rows as PR
import pyref as P
import recover_rows as RR

# where a fault CAN show: the folds need a round; sh_pz[0] is read as such at m = 1 alone
FAULT_KS = {
    "halves_swapped": range(1, 13), "y_power_sign": range(1, 13), "dR_slot": range(1, 13), "e_swap_b": range(1, 13),
    "pz_m1": range(0, 7), "amount_i32": range(0, 13), "alpha_no_y": range(0, 13),
}


def test_row_table():
    for k in RR.KS:
        for n, m in RR.shapes(k):
            names = PR.row_names(n, m)
            assert len(names) == len(set(names)) == (3 if k >= PR.CAPPED_FROM_K else 33)
            rows = PR.shape_rows("secp256k1", n, m)
            r = rows[0].r
            for row in rows:
                assert len(row.values) == len(row.gammas) == m and all(0 <= v < 1 << 64 for v in row.values)
                assert all(0 <= x < r for x in row.gammas + row.ch_values() + row.blind_values())
                assert len(row.ch_values()) == 3 + k and len(row.blind_values()) == 5 + 2 * k
                assert row.ch_values()[0] and all(row.ch_values()[3:])          # y and every e_t: non-zero
            if k < PR.CAPPED_FROM_K:
                tops = [row.ch for row in rows if row.name.startswith("top(")]
                for s in range(3 + k):   # every top value on y, on z, on e and on every e_t
                    assert {ch[s] for ch in tops} == set(RR.top_values(r))
            else:
                assert set(RR.top_values(r)) <= set(rows[1].ch)


@pytest.mark.parametrize("cname", PR.CURVES)
def test_model_a_equals_model_b_on_every_row(cname):
    rows = PR.corpus(cname)
    assert {row.k for row in rows} == set(range(13))
    for row in rows:
        pa, ta = PR.expected(row.cname, row.n, row.m, row.name)
        pb, tb = PR.model_b(row)
        assert ta == tb, row
        assert pa == pb, (row, [v for v, (x, y) in enumerate(zip(pa, pb)) if x != y])
        assert len(pa) == PR.num_vps(row.k, row.m)


def test_what_the_edge_rows_are_for():
    """zero_a: c_L = c_R = 0 in every round and r' = r ; identity: V has no term at all ; e_zero: the triple is [r, s, eta]"""
    for n, m in ((8, 1), (1, 8), (64, 4), (64, 64)):
        for name in ("zero_a(z=0)", "zero_a(z=1)")[0 if n * m < 512 else 1:]:
            row = PR.make_row("bls12_381", n, m, name)
            pts, triple = PR.expected("bls12_381", n, m, name)
            assert all(0 not in pts[v] for v in range(1, 2 * row.k + 1)) and triple[0] == row.blind_values()[1]
        if n * m < 512:
            pts, _ = PR.expected("bls12_381", n, m, "identity")
            assert all(p == {} for p in pts[-m:])
            row = PR.make_row("bls12_381", n, m, "e_zero")
            assert PR.expected("bls12_381", n, m, "e_zero")[1] == [row.blind[1], row.blind[2], row.blind[4]]


def test_every_fault_changes_an_output_at_every_k_where_it_can():
    cname = "secp256k1"
    for fault in PR.FAULTS:
        for k in RR.KS:
            hit = None
            for row in PR.corpus(cname, (k,)):
                if PR.model_b(row, fault) != PR.expected(row.cname, row.n, row.m, row.name):
                    hit = row
                    break
            assert (hit is not None) == (k in FAULT_KS[fault]), (fault, k, hit)
            if fault == "pz_m1" and hit is not None:
                assert hit.m == 1


@pytest.mark.parametrize("cname", PR.CURVES)
def test_forward_delta_prime_of_recover_rows(cname):
    for row in PR.corpus(cname):
        want = RR.delta_prime(row.r, row.n, row.m, row.ch_values(), row.blind_values(), row.gammas)
        assert PR.expected(row.cname, row.n, row.m, row.name)[1][2] == want, row


@pytest.mark.parametrize("cname,n,m", [("bls12_381", 8, 1), ("secp256k1", 1, 8), ("ed25519", 4, 4), ("bls12_381", 64, 2)])
def test_literals_equal_pyref_shadow_prover(cname, n, m):
    """dlog of g, h, G_i, H_i in pyref.PublicKey: 1, 2, 3 (i + 1), 5 (i + 1) -- a shadow point is sum c_f dlog(f)"""
    row = PR.make_row(cname, n, m, "literal")
    assert row.ch is None and row.blind is None and not row.flag
    pts, triple = PR.expected(cname, n, m, "literal")
    _, prover, proof = P.prove_case(cname, n, row.values, row.gammas, shadow=True)
    w = proof.proof
    assert triple == [w.r_prime, w.s_prime, w.d_prime]
    mn, k = n * m, row.k
    dlog = [1, 2] + [3 * (i + 1) for i in range(mn)] + [5 * (i + 1) for i in range(mn)]
    shadow = [sum(c * dlog[f] for f, c in p.items()) % row.r for p in pts]
    want = [proof.A] + [x for LR in zip(w.L_vec, w.R_vec) for x in LR] + [w.A, w.B] + list(prover.commitment_vec)
    assert shadow == want and len(want) == PR.num_vps(k, m)
