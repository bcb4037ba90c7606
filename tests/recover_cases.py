"""Mask recovery: the big-integer statement of what csrc/recover_terms.hpp computes, and oracle-made proofs to recover
from.  With [y, z, e, e_1..e_k] the challenge block of a proof of shape (n, m), k = log2(n m), and its blinding scalars
[alpha, r, s, delta, eta, d_L[0..k), d_R[0..k)] (reference src/range/mod.rs:159-172, :366-376;
src/weighted_inner_product_proof.rs:94-95, :171, :175-227):

    alpha_k = (delta' - eta - delta e) e^-2
    S       = (alpha_k - sum_t (e_t^2 d_L[t] + e_t^-2 d_R[t]) - alpha) y^-(nm+1)
    Gamma   = S (m = 1) or S z^-2 (m > 1)  =  gamma_0 + z^2 gamma_1 + .. + z^(2(m-1)) gamma_{m-1}

The EXPECTED value of a test is gamma_of(): from the gammas the test chose and the z the oracle drew -- never from the
library, and not from recover_bigint either (that one restates the inversion; the CPU test holds it against gamma_of)."""

import numpy as np

import oracle as O
import pyref as P

ORDER = {name: P.CURVES[name]["r"] for name in ("bls12_381", "secp256k1", "ed25519")}


def literal_challenges(n, m):
    """the reference's constants [y, z, e, e_1..e_k] (range/mod.rs:198-199 / :417-418, wip.rs:353, :369)"""
    k = (n * m).bit_length() - 1
    return ([7, 7] if m == 1 else [12, 23]) + [99] + [7] * k


def literal_blinding(n, m):
    """the reference's literal blinding scalars in the prover's layout (range/mod.rs:94 / :256, wip.rs:94-95, :175-178)"""
    k = (n * m).bit_length() - 1
    return [7 if m == 1 else 33, 33, 44, 88, 123] + [4] * k + [5] * k


def gamma_of(r, gammas, z):
    """Gamma = sum_j z^(2j) gamma_j"""
    return sum(pow(z, 2 * j, r) * g for j, g in enumerate(gammas)) % r


def recover_bigint(r, n, m, dprime, ch, blind):
    k = (n * m).bit_length() - 1
    assert len(ch) == 3 + k and len(blind) == 5 + 2 * k
    y, z, e, et = ch[0], ch[1], ch[2], ch[3:]
    alpha, delta, eta, dL, dR = blind[0], blind[3], blind[4], blind[5:5 + k], blind[5 + k:]
    inv = lambda x: pow(x, r - 2, r)
    a = (dprime - eta - delta * e) * inv(e * e) % r
    for t in range(k):
        a -= et[t] * et[t] * dL[t] + inv(et[t] * et[t]) * dR[t]
    s = (a - alpha) * inv(pow(y, n * m + 1, r)) % r
    return s if m == 1 else s * inv(z * z) % r


def oracle_proof(cname, n, values, gammas, transcript, blind=None):
    """One proof by the C oracle's prover (BLS12-381, secp256k1).  blind: None (the literals) or the 5 + 2k scalars.
    -> dict: points (3 + 2k, PW), scalars (3, 4), V (m, PW), ch [ints] (the oracle's own in transcript mode, the literals
    otherwise: want_challenges returns zeros there), blind [ints]"""
    curve = O.CURVE_IDS[cname]
    m = len(values)
    pk = O.PublicKey(curve, n * m)
    O.set_transcript(transcript)
    O.set_blinding(blind)
    try:
        pts, sc, V = O.range_prove(pk, n, values, gammas)
        rc, _, _, ch = O.range_verify(pk, n, m, pts, sc, V, want_challenges=True)
    finally:
        O.set_transcript(False)
        O.set_blinding(None)
    assert rc == 0, "the oracle rejects its own proof"
    chal = O.wire_to_scalars(ch) if transcript else literal_challenges(n, m)
    return {"n": n, "m": m, "points": pts, "scalars": sc, "V": V, "ch": [int(x) for x in chal],
            "blind": list(blind) if blind is not None else literal_blinding(n, m),
            "triple": [int(x) for x in O.wire_to_scalars(sc)]}


def record(proof):
    """the verification record [A, wip.A, wip.B, L.., R.., V_0..] of an oracle proof"""
    return np.concatenate([proof["points"], proof["V"]])
