"""CPU: mask recovery (csrc/recover_terms.hpp) through its host build (tests/host/recover_host_test.cpp, the code
k_recover_masks runs, term after term).  The proofs are the C oracle's -- secp256k1 and BLS12-381, shapes (8,1), (8,2),
(8,4), (16,1), under the transcript with the blinding expanded from a key (oracle.blinding_from_key) and in the reference's
literal mode -- and the expected Gamma is gamma_0 + z^2 gamma_1 + .. from the gammas chosen here and the oracle's z
(recover_cases.gamma_of).  A wrong key, an index off by one and a flipped bit of delta' each give another value.
BPP_HOST_SANITIZE=1 builds the program under ASan + UBSan (a stand-alone binary, like the other host tests)."""

import random

import subprocess

import pytest

import recover_cases as RC
import recover_rows as RR
from test_host_arith_cpu import _build

CID = {"bls12_381": 0, "secp256k1": 1, "ed25519": 2}
SHAPES = ((8, 1), (8, 2), (8, 4), (16, 1))
KEY = bytes(range(7, 39))
INDEX0 = (1 << 33) + 5


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build("recover_host_test", tmp_path_factory.mktemp("host"), "-O2")


def _hex(x):
    return "%064x" % x


def _line(cname, p, source):
    k = (p["n"] * p["m"]).bit_length() - 1
    return " ".join([str(CID[cname]), str(k), str(p["m"])] + source + [_hex(x) for x in p["triple"]] + [_hex(x) for x in p["ch"]])


def _run(harness, tmp_path, lines):
    f = tmp_path / "proofs.txt"
    f.write_text("\n".join(lines) + "\n")
    out = subprocess.run([harness, str(f)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    return [(int(g, 16), int(ok)) for g, ok in rows]


def _inputs(cname, seed):
    r = RC.ORDER[cname]
    rng = random.Random(seed)
    out = []
    for j, (n, m) in enumerate(SHAPES):
        values = [rng.randrange(1 << n) for _ in range(m)]
        gammas = [rng.randrange(1, r) for _ in range(m)]
        if j == 0:
            gammas[0] = r - 1
        out.append((n, values, gammas))
    return out


@pytest.fixture(scope="module")
def keyed():
    """{curve: [(proof, gammas, index)]}: transcript mode, blinding from (KEY, INDEX0 + j)"""
    made = {}
    for cname in ("secp256k1", "bls12_381"):
        r = RC.ORDER[cname]
        made[cname] = []
        for j, (n, values, gammas) in enumerate(_inputs(cname, 4100 + CID[cname])):
            k = (n * len(values)).bit_length() - 1
            proof = RC.oracle_proof(cname, n, values, gammas, True, RC.O.blinding_from_key(KEY, INDEX0 + j, k, r))
            made[cname].append((proof, gammas, INDEX0 + j))
    return made


@pytest.mark.parametrize("cname", ["secp256k1", "bls12_381"])
def test_key_derived_blinding_under_the_transcript(harness, tmp_path, keyed, cname):
    r = RC.ORDER[cname]
    proofs = keyed[cname]
    want = [RC.gamma_of(r, gammas, p["ch"][1]) for p, gammas, _ in proofs]
    for (p, gammas, _), w in zip(proofs, want):   # the big-integer formula agrees with the chosen masks
        assert RC.recover_bigint(r, p["n"], p["m"], p["triple"][2], p["ch"], p["blind"]) == w
        if p["m"] == 1:
            assert w == gammas[0]
    got = _run(harness, tmp_path, [_line(cname, p, ["key", KEY.hex(), str(idx)]) for p, _, idx in proofs])
    assert got == [(w, 1) for w in want]
    # the same scalars handed over as a blinding buffer
    got = _run(harness, tmp_path, [_line(cname, p, ["blind"] + [_hex(x) for x in p["blind"]]) for p, _, _ in proofs])
    assert got == [(w, 1) for w in want]


@pytest.mark.parametrize("cname", ["secp256k1", "bls12_381"])
def test_literal_mode(harness, tmp_path, cname):
    r = RC.ORDER[cname]
    lines, want = [], []
    for n, values, gammas in _inputs(cname, 4200 + CID[cname]):
        p = RC.oracle_proof(cname, n, values, gammas, False)
        lines.append(_line(cname, p, ["lit"]))
        want.append(RC.gamma_of(r, gammas, p["ch"][1]))
    assert _run(harness, tmp_path, lines) == [(w, 1) for w in want]


@pytest.mark.parametrize("cname", ["secp256k1", "bls12_381"])
def test_wrong_key_wrong_index_flipped_bit(harness, tmp_path, keyed, cname):
    r = RC.ORDER[cname]
    lines, want = [], []
    other = bytes(KEY[:-1]) + bytes([KEY[-1] ^ 1])
    for p, gammas, idx in keyed[cname]:
        w = RC.gamma_of(r, gammas, p["ch"][1])
        flipped = dict(p, triple=p["triple"][:2] + [p["triple"][2] ^ 1])
        lines += [_line(cname, p, ["key", other.hex(), str(idx)]), _line(cname, p, ["key", KEY.hex(), str(idx + 1)]),
                  _line(cname, p, ["key", KEY.hex(), str(idx - 1)]), _line(cname, flipped, ["key", KEY.hex(), str(idx)])]
        want += [w] * 4
    got = _run(harness, tmp_path, lines)
    for (g, ok), w in zip(got, want):
        assert ok == 1 and g != w and g < r


def test_zero_challenge_gives_zero(harness, tmp_path, keyed):
    """an inversion that is not defined: Gamma = 0 and the flag is down -- for e, y, a round challenge, and z when m > 1;
    z = 0 with m = 1 does not enter"""
    lines, want_zero = [], []
    for p, _, idx in keyed["secp256k1"]:
        k = (p["n"] * p["m"]).bit_length() - 1
        for pos in (0, 1, 2, 3, 2 + k):
            ch = list(p["ch"])
            ch[pos] = 0
            lines.append(_line("secp256k1", dict(p, ch=ch), ["key", KEY.hex(), str(idx)]))
            want_zero.append(not (pos == 1 and p["m"] == 1))
    got = _run(harness, tmp_path, lines)
    for (g, ok), z in zip(got, want_zero):
        assert (g == 0 and ok == 0) if z else ok == 1


def test_edwards_scalar_field(harness, tmp_path):
    """the third scalar field (no C oracle prover there): delta' built by the formula's inverse from chosen gammas"""
    cname, r = "ed25519", RC.ORDER["ed25519"]
    rng = random.Random(77)
    lines, want = [], []
    for n, m in SHAPES:
        k = (n * m).bit_length() - 1
        ch = [rng.randrange(1, r) for _ in range(3 + k)]
        blind = RC.O.blinding_from_key(KEY, 9 + k, k, r)
        gammas = [rng.randrange(r) for _ in range(m)]
        z = ch[1]
        dprime = RR.delta_prime(r, n, m, ch, blind, gammas)   # forward, in the prover's direction
        p = {"n": n, "m": m, "triple": [1, 2, dprime], "ch": ch}
        lines.append(_line(cname, p, ["key", KEY.hex(), str(9 + k)]))
        want.append(RC.gamma_of(r, gammas, z))
    assert _run(harness, tmp_path, lines) == [(w, 1) for w in want]
