"""CPU: the corpus of synthetic recovery rows (tests/recover_rows.py) and what holds it.

Every row's delta' is built forward, in the prover's direction, and its expected Gamma is gamma_of(gammas, z).  Here
  - the inverse direction (recover_cases.recover_bigint) and the many-key closed forms (recover_rows.coeff_closed_forms)
    must give the same Gamma on every row whose inversions are defined;
  - the whole corpus, k = 0..12 on three curves, runs through the product's headers on the host: recover_host_test
    (recover_terms.hpp, a key row as "key" and as "blind", a buffer row as "blind") and recover_keys_host_test
    (recover_coeffs.hpp; its line format carries keys, so the key rows, each under the owner and two foreign keys);
  - the census: per curve and k every challenge position occurs zeroed, with m = 1 and with m > 1 wherever k allows both,
    every top value and every blinding edge occurs, and no row is missing: a row the builder cannot make raises.
BPP_HOST_SANITIZE=1 builds both programs under ASan + UBSan (stand-alone binaries, like the other host tests)."""

import functools
import subprocess

import pytest

import recover_cases as RC
import recover_rows as RR
from test_host_arith_cpu import _build

CID = {"bls12_381": 0, "secp256k1": 1, "ed25519": 2}
KEYS = [RR.OWNER, RR.FOREIGN[0], RR.FOREIGN[1]]


@functools.lru_cache(maxsize=None)
def _corpus(cname, source):
    return tuple(RR.corpus(cname, source))


@pytest.fixture(scope="module")
def terms_harness(tmp_path_factory):
    return _build("recover_host_test", tmp_path_factory.mktemp("host"), "-O2")


@pytest.fixture(scope="module")
def keys_harness(tmp_path_factory):
    return _build("recover_keys_host_test", tmp_path_factory.mktemp("host"), "-O2")


def _hex(x):
    return "%064x" % x


def _tail(row):
    return [_hex(x) for x in row.triple] + [_hex(x) for x in row.ch]


def _run(harness, tmp_path, lines, per_line):
    f = tmp_path / "rows.txt"
    f.write_text("\n".join(lines) + "\n")
    out = subprocess.run([harness, str(f)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = [ln.split() for ln in out.stdout.splitlines()]
    assert len(got) == len(lines) * per_line
    return got


@pytest.mark.parametrize("source", RR.SOURCES)
@pytest.mark.parametrize("cname", RR.CURVES)
def test_forward_and_inverse_directions_agree(cname, source):
    r = RC.ORDER[cname]
    rows = _corpus(cname, source)
    n_defined = 0
    for row in rows:
        assert 0 <= row.gamma < r and len(row.ch) == 3 + row.k and len(row.blind) == 5 + 2 * row.k
        if row.bad:
            assert row.gamma == 0 and RR.is_zero_name(row.name) and 0 in row.ch
            continue
        n_defined += 1
        assert RC.recover_bigint(r, row.n, row.m, row.triple[2], row.ch, row.blind) == row.gamma, row
        co = RR.coeff_closed_forms(r, row.n, row.m, row.triple[2], row.ch)
        assert len(co) == 2 * row.k + 4 and RR.gamma_by_coeffs(r, co, row.blind) == row.gamma, row
        if row.m == 1:
            assert row.gamma == row.gammas[0]
        if row.name == "gamma_zero":
            assert row.gamma == 0 and 0 not in row.ch
        if row.name.startswith("delta_edges("):
            assert row.triple[2] == int(row.name[12:-1]) % r
    assert n_defined > len(rows) // 2


@pytest.mark.parametrize("cname", RR.CURVES)
def test_census(cname):
    r = RC.ORDER[cname]
    for source in RR.SOURCES:
        rows = _corpus(cname, source)
        by_k = {k: [row for row in rows if row.k == k] for k in RR.KS}
        assert sum(len(v) for v in by_k.values()) == len(rows)
        for k in RR.KS:
            shapes = RR.shapes(k)
            assert shapes and all(n * m == 1 << k and n <= 64 and m <= 64 for n, m in shapes), k
            # both kinds of shape wherever n, m <= 64 allows both: m = 1 needs n = 2^k <= 64, m > 1 needs k >= 1
            assert any(m == 1 for _, m in shapes) == (k <= 6) and any(m > 1 for _, m in shapes) == (k >= 1), k
            # no row skipped: every name of every shape, once
            for n, m in shapes:
                names = [row.name for row in by_k[k] if (row.n, row.m) == (n, m)]
                assert names == RR.row_names(k, source), (cname, k, n, m)
            for kind in ({1} if k == 0 else {1, 2} if k <= 6 else {2}):
                of_kind = [row for row in by_k[k] if (row.m == 1) == (kind == 1)]
                zeroed = {row.ch.index(0) for row in of_kind if RR.is_zero_name(row.name)}
                assert zeroed == set(range(3 + k)), (cname, source, k, kind, zeroed)
                for row in of_kind:
                    if RR.is_zero_name(row.name):
                        assert row.ch.count(0) == 1
                        assert row.bad == (not (row.m == 1 and row.ch[1] == 0))
            tops = {x for row in by_k[k] if row.name.startswith("top(") for x in row.ch}
            assert tops == set(RR.top_values(r)), (cname, k)
            assert all(set(row.ch) == {r - 1} for row in by_k[k] if row.name == "minus_one")
            assert all(set(row.ch) == {1} for row in by_k[k] if row.name == "one")
            if source == "buffer":
                for n, m in shapes:
                    edges = [row.blind for row in by_k[k] if (row.n, row.m) == (n, m) and row.name.startswith("blind_edges(")]
                    for s in range(5 + 2 * k):
                        if s not in (1, 2):
                            assert {b[s] for b in edges} == {0, 1, r - 1}
    with pytest.raises(ValueError):   # a row the builder cannot make is an error, not a skip
        RR.make_row(cname, 8, 1, "zero(e_3)", "buffer")
    with pytest.raises(ValueError):
        RR.make_row(cname, 8, 1, "blind_edges(0)", "key")


@pytest.mark.parametrize("cname", RR.CURVES)
def test_terms_through_the_host_build(terms_harness, tmp_path, cname):
    """recover_mask of csrc/recover_terms.hpp, the code k_recover_masks runs term after term, on every row"""
    lines, rows = [], []
    for row in _corpus(cname, "key"):
        head = [str(CID[cname]), str(row.k), str(row.m)]
        lines.append(" ".join(head + ["key", row.key.hex(), str(row.index)] + _tail(row)))
        lines.append(" ".join(head + ["blind"] + [_hex(x) for x in row.blind] + _tail(row)))
        rows += [row, row]
    for row in _corpus(cname, "buffer"):
        lines.append(" ".join([str(CID[cname]), str(row.k), str(row.m), "blind"] + [_hex(x) for x in row.blind] + _tail(row)))
        rows.append(row)
    got = _run(terms_harness, tmp_path, lines, 1)
    wrong = [(row, g) for row, (g, ok) in zip(rows, got) if (int(g, 16), int(ok)) != (row.gamma, 0 if row.bad else 1)]
    assert not wrong, "%d of %d rows, first %r" % (len(wrong), len(rows), wrong[:4])


@pytest.mark.parametrize("cname", RR.CURVES)
def test_coefficients_through_the_host_build(keys_harness, tmp_path, cname):
    """recover_coeffs and the strided sum of csrc/recover_coeffs.hpp on every key row, under the owner and two foreign
    keys: the owner reads the chosen Gamma, a foreign key what the closed forms give on ITS expansion, a zero row zero"""
    rows = _corpus(cname, "key")
    lines = [" ".join([str(CID[cname]), str(row.k), str(row.m), str(row.index), str(len(KEYS))] + [key.hex() for key in KEYS] +
                      _tail(row)) for row in rows]
    got = _run(keys_harness, tmp_path, lines, len(KEYS))
    wrong = []
    for i, row in enumerate(rows):
        ok = 0 if row.bad else 1
        want = [row.gamma] + [0 if row.bad else RR.foreign_gamma(row, key, row.index) for key in KEYS[1:]]
        if not row.bad:
            assert len(set(want)) == 3
        for (g, by_mask, ok1, ok2, rs_zero), w in zip(got[i * len(KEYS):(i + 1) * len(KEYS)], want):
            if (int(g, 16), int(by_mask, 16), int(ok1), int(ok2)) != (w, w, ok, ok) or (ok and int(rs_zero) != 1):
                wrong.append((row, g))
    assert not wrong, "%d pairs of %d rows, first %r" % (len(wrong), len(rows), wrong[:4])
