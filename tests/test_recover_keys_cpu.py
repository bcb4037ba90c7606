"""CPU: the key-independent coefficients of mask recovery and the projective comparison of the many-key scan
(csrc/recover_coeffs.hpp) through their host build (tests/host/recover_keys_host_test.cpp: the code k_recover_coeffs,
k_scan_keys and k_scan_keys_confirm run, through pair_gamma and pair_confirms, which the find kernels call too).

Gamma = A0 + sum_s c_s slot_s(key, index) is held against recover_mask's output (the single-key code) AND against the
big-integer value recover_cases.recover_bigint on oracle.blinding_from_key(key, index, k, r) -- for the owning key also
against gamma_0 + z^2 gamma_1 + .. from the gammas chosen here (recover_cases.gamma_of).  The proofs are the C oracle's
(secp256k1, BLS12-381; shapes (8,1), (8,2), (8,4), (16,1)); on the Edwards scalar field delta' is built by the formula's
inverse.  Each proof is read under the owning key and two foreign keys.  BPP_HOST_SANITIZE=1 builds the program under
ASan + UBSan (a stand-alone binary, like the other host tests)."""

import hashlib
import random
import subprocess

import pytest

import recover_cases as RC
import recover_rows as RR
from test_host_arith_cpu import _build

CID = {"bls12_381": 0, "secp256k1": 1, "ed25519": 2}
SHAPES = ((8, 1), (8, 2), (8, 4), (16, 1))
KEYS = [bytes(range(7, 39)), hashlib.sha256(b"a foreign view key").digest(), hashlib.sha256(b"another foreign view key").digest()]
INDEX0 = (1 << 33) + 5


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build("recover_keys_host_test", tmp_path_factory.mktemp("host"), "-O2")


def _hex(x):
    return "%064x" % x


def _line(cname, p, index, keys):
    k = (p["n"] * p["m"]).bit_length() - 1
    return " ".join([str(CID[cname]), str(k), str(p["m"]), str(index), str(len(keys))] + [key.hex() for key in keys] +
                    [_hex(x) for x in p["triple"]] + [_hex(x) for x in p["ch"]])


def _run(harness, tmp_path, lines, n_keys):
    f = tmp_path / "proofs.txt"
    f.write_text("\n".join(lines) + "\n")
    out = subprocess.run([harness, str(f)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines()]
    assert len(rows) == len(lines) * n_keys
    rows = [(int(g, 16), int(w, 16), int(ok), int(ok2), int(z)) for g, w, ok, ok2, z in rows]
    return [rows[i * n_keys:(i + 1) * n_keys] for i in range(len(lines))]


@pytest.fixture(scope="module")
def keyed():
    """{curve: [(proof, gammas, index)]}: the oracle's proofs under the transcript, blinding from (KEYS[0], INDEX0 + j)"""
    made = {}
    for cname in ("secp256k1", "bls12_381"):
        r = RC.ORDER[cname]
        rng = random.Random(4300 + CID[cname])
        made[cname] = []
        for j, (n, m) in enumerate(SHAPES):
            values = [rng.randrange(1 << n) for _ in range(m)]
            gammas = [rng.randrange(1, r) for _ in range(m)]
            k = (n * m).bit_length() - 1
            proof = RC.oracle_proof(cname, n, values, gammas, True, RC.O.blinding_from_key(KEYS[0], INDEX0 + j, k, r))
            made[cname].append((proof, gammas, INDEX0 + j))
    return made


def _bigint(cname, p, key, index):
    r = RC.ORDER[cname]
    k = (p["n"] * p["m"]).bit_length() - 1
    return RC.recover_bigint(r, p["n"], p["m"], p["triple"][2], p["ch"], RC.O.blinding_from_key(key, index, k, r))


@pytest.mark.parametrize("cname", ["secp256k1", "bls12_381"])
def test_coefficients_reproduce_gamma_for_every_key(harness, tmp_path, keyed, cname):
    r = RC.ORDER[cname]
    proofs = keyed[cname]
    got = _run(harness, tmp_path, [_line(cname, p, idx, KEYS) for p, _, idx in proofs], len(KEYS))
    for (p, gammas, idx), rows in zip(proofs, got):
        want = [_bigint(cname, p, key, idx) for key in KEYS]
        assert want[0] == RC.gamma_of(r, gammas, p["ch"][1])   # the owner reads the chosen masks
        assert want[1] != want[0] and want[2] != want[0] and want[1] != want[2]
        for (g, by_mask, ok, ok2, rs_zero), w in zip(rows, want):
            assert (g, by_mask, ok, ok2) == (w, w, 1, 1)
            assert rs_zero == 1   # c_r = c_s = 0: those slots are never hashed


def test_edwards_scalar_field(harness, tmp_path):
    """the third scalar field (no C oracle prover there): delta' built by the formula's inverse from chosen gammas"""
    cname, r = "ed25519", RC.ORDER["ed25519"]
    rng = random.Random(79)
    lines, want = [], []
    for n, m in SHAPES:
        k = (n * m).bit_length() - 1
        ch = [rng.randrange(1, r) for _ in range(3 + k)]
        index = 9 + k
        blind = RC.O.blinding_from_key(KEYS[0], index, k, r)
        gammas = [rng.randrange(r) for _ in range(m)]
        z = ch[1]
        dprime = RR.delta_prime(r, n, m, ch, blind, gammas)   # forward, in the prover's direction
        p = {"n": n, "m": m, "triple": [1, 2, dprime], "ch": ch}
        lines.append(_line(cname, p, index, KEYS))
        w = [_bigint(cname, p, key, index) for key in KEYS]
        assert w[0] == RC.gamma_of(r, gammas, z)
        want.append(w)
    got = _run(harness, tmp_path, lines, len(KEYS))
    for rows, w in zip(got, want):
        assert [(g, m_) for g, m_, _, _, _ in rows] == [(x, x) for x in w]
        assert all(ok == 1 and ok2 == 1 and z == 1 for _, _, ok, ok2, z in rows)


def test_zero_challenge_is_undefined(harness, tmp_path, keyed):
    """ok = false exactly where recover_mask's flag is down: e, y, a round challenge, and z when m > 1; z = 0 with m = 1
    does not enter"""
    lines, want_zero = [], []
    for p, _, idx in keyed["secp256k1"]:
        k = (p["n"] * p["m"]).bit_length() - 1
        for pos in (0, 1, 2, 3, 2 + k):
            ch = list(p["ch"])
            ch[pos] = 0
            lines.append(_line("secp256k1", dict(p, ch=ch), idx, KEYS[:1]))
            want_zero.append(not (pos == 1 and p["m"] == 1))
    got = _run(harness, tmp_path, lines, 1)
    for rows, z in zip(got, want_zero):
        g, by_mask, ok, ok2, _ = rows[0]
        assert ok == ok2 == (0 if z else 1)
        assert g == by_mask and (g == 0) == z


def test_projective_comparison_agrees_with_the_inversion(harness):
    """walk_equals_wire against jac_to_aff + the wire comparison of k_recover_confirm: equal and unequal points, infinity
    on either side and on both, an accumulator that cancelled to the identity; edwards25519: representatives shifted by
    the three non-trivial points of E[4] are the same element, the next multiple of g is not"""
    out = subprocess.run([harness, "cmp"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = dict(ln.split()[2:4] for ln in out.stdout.splitlines() if ln.startswith("ok cmp"))
    assert set(got) == {"bls12_381", "secp256k1", "ed25519"}
    assert int(got["bls12_381"]) == int(got["secp256k1"]) == 110 and int(got["ed25519"]) == 110 + 60
