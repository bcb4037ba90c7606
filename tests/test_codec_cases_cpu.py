"""CPU: the case builder of the codec tests (tests/codec_cases.py) is itself right, and csrc/ristretto.hpp equals the
restatement in a host build.

 * every tracing twin equals the pyref function it shadows on its whole corpus;
 * the CENSUS: the corpora reach every branch combination they claim to -- all 32 traces of rist_decode and of rist_encode,
   all 8 of MAP, every rejection reason, both verdicts and both flags of each x sweep, try-and-increment counters past 0
   and both parity outcomes in the hashed keys, points on both sides of (p - 1) / 2 and at every word step from it.  The
   GPU tests (tests/test_gpu_codec_cases.py) compare the device with the restatement on these corpora; the census is what
   makes that comparison a statement about branches.  A count that comes out low means a larger corpus, not a lower bar;
 * tests/host/ristretto_host_test.cpp -- csrc/ristretto.hpp under g++ (ASan + UBSan with BPP_HOST_SANITIZE=1, a
   stand-alone binary like the other host tests) -- on the whole decode and encode corpora, on rist_equal, and on the
   inputs of rist_from_uniform_bytes that the ABI cannot deliver (t >= p, bit 255 set), bit for bit against pyref."""

import collections
import itertools
import os
import subprocess

import pytest

import codec_cases as CC
import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = P.Ristretto255

# BPP_HOST_SANITIZE=1: host builds under ASan + UBSan (see tests/test_host_arith_cpu.py)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("BPP_HOST_SANITIZE") else []

OUTCOMES = ("correct", "flipped", "flipped_i", "none")
BOOLS = (False, True)


# ---- the twins equal what they shadow ----------------------------------------------------------------------------------
def test_decode_twin_equals_the_restatement():
    cases = CC.rist_decode_cases()
    assert len(cases) == 400 + 4 + 3 + 4 + 3 + 1
    for c in cases:
        assert CC.decode_traced(c.data) == (c.point, c.trace, c.reason) and c.point == R.decode(c.data), c.data.hex()
        assert (c.point is None) == (c.reason is not None)
        assert P.decompress_point(P.ED25519, c.data) == (c.point is not None, c.point)


def test_encode_twin_equals_the_restatement():
    G = CC._edwards()
    cases = CC.rist_encode_cases()
    assert len(cases) == 4 * (1 + 64 + 1 + 16)
    for c in cases:
        assert G.on_curve(c.point) and CC.encode_traced(c.point) == (c.data, c.trace) and c.data == R.encode(c.point), c.note
    # the four representatives of a coset share one encoding, which decodes to a representative of the same coset
    for _, grp in itertools.groupby(cases, key=lambda c: c.coset):
        grp = list(grp)
        assert len(grp) == 4 and len({c.data for c in grp}) == 1 and len({c.point for c in grp}) == 4
        back = R.decode(grp[0].data)
        assert back is not None and all(R.equal(back, c.point) for c in grp)
    assert cases[0].point == (0, 1) and cases[0].data == bytes(32)
    assert cases[4].point == G.base() and cases[4].data == R.BASE_ENCODING
    assert len({c.data for c in cases}) == len(cases) // 4


def test_sqrt_ratio_and_map_twins_equal_the_restatement():
    G = CC._edwards()
    for b in CC.uniform_cases():
        pt, maps = CC.from_uniform_bytes_traced(b, G)
        assert pt == R.from_uniform_bytes(b, G)
        for h in range(2):
            t = (int.from_bytes(b[32 * h:32 * h + 32], "little") & ((1 << 255) - 1)) % R.P
            assert CC.map_traced(t)[0] == R.map(t)
            r = R.SQRT_M1 * t * t % R.P
            u, v = (r + 1) * R.ONE_MINUS_D_SQ % R.P, (-1 - r * R.D) * (r + R.D) % R.P
            assert CC.sqrt_ratio_m1_traced(u, v)[:2] == R.sqrt_ratio_m1(u, v)
    for u, v in ((0, 0), (0, 5), (5, 0), (1, 1), (1, R.P - 1), (1, R.SQRT_M1), (1, R.P - R.SQRT_M1), (4, 9)):
        assert CC.sqrt_ratio_m1_traced(u, v)[:2] == R.sqrt_ratio_m1(u, v)


@pytest.mark.parametrize("cname", ["bls12_381", "secp256k1", "ed25519"])
def test_hash_to_group_twin_equals_the_restatement_and_is_prefix_stable(cname):
    curve = P.CURVES[cname]
    G = CC._edwards() if cname == "ed25519" else P.WeierstrassGroup(curve)
    keys = CC.hashed_key_cases(cname)
    assert [(lb, ln) for lb, ln, _ in keys] == list(CC.KEYS)
    for label, length, pts in keys:
        ids = [("h", 0)] + [("G", i) for i in range(length)] + [("H", i) for i in range(length)]
        assert len(pts) == 1 + 2 * length
        for (kind, idx), hp in zip(ids, pts):
            assert hp.point == P.hash_to_group(curve, G, label, kind, idx), (label, kind, idx)
            assert G.on_curve(hp.point)
    # the prefix property (csrc/mixed.hpp relies on it): hash_to_group(.., idx) takes no length, so the key of length 8
    # is h, G_0..7, H_0..7 of the key of length 40
    (_, _, long), (_, _, short) = keys[0], keys[1]
    assert short[0] == long[0] and short[1:9] == long[1:9] and short[9:17] == long[41:49]
    every = [hp.point for _, _, pts in keys[:1] + keys[2:] for hp in pts]
    assert len(set(every)) == len(every)          # distinct labels, distinct generators


# ---- the census ---------------------------------------------------------------------------------------------------------
def test_census_of_the_ristretto_corpora():
    dec = collections.Counter(c.trace for c in CC.rist_decode_cases() if c.trace is not None)
    want = set(itertools.product(OUTCOMES, BOOLS, BOOLS, BOOLS))
    assert set(dec) == want and min(dec.values()) >= 3, sorted(dec.items(), key=lambda kv: kv[1])[:4]
    reasons = collections.Counter(c.reason for c in CC.rist_decode_cases())
    assert set(reasons) == set(CC.REASONS) | {None} and reasons[None] >= 100
    # the single points of the input space
    by_s = {int.from_bytes(c.data, "little"): c for c in CC.rist_decode_cases()}
    p = R.P
    assert by_s[p - 1].reason == "y = 0" and by_s[0].point == (0, 1)
    assert [by_s[s].reason for s in (p, p + 1, p + 18, (1 << 255) - 1)] == ["non-canonical"] * 4
    assert [by_s[s].reason for s in (1 << 255, (1 << 255) + 2, (1 << 256) - 2)] == ["bit 255 set"] * 3
    assert reasons["bit 255 set"] == 4
    masked = [c for c in CC.rist_decode_cases() if c.reason == "bit 255 set"]
    below = [R.decode((int.from_bytes(c.data, "little") - (1 << 255)).to_bytes(32, "little")) for c in masked]
    assert sum(q is not None for q in below) >= 2                         # strings with nothing wrong but bit 255
    assert [by_s[s].reason for s in (1, 3, p - 2)] == ["negative s"] * 3

    enc = collections.Counter(c.trace for c in CC.rist_encode_cases())
    want = set(itertools.product(("correct", "flipped"), BOOLS, BOOLS, BOOLS, BOOLS))
    assert want <= set(enc) and min(enc[t] for t in want) >= 3, sorted(enc.items(), key=lambda kv: kv[1])[:4]
    # what is outside the 32: the points of E[4] (x y = 0, the square root of 0)
    assert {c.coset for c in CC.rist_encode_cases() if c.trace not in want} == {0}


def test_census_of_the_weierstrass_corpora():
    for cname in ("bls12_381", "secp256k1"):
        curve = P.CURVES[cname]
        p = curve["p"]
        cases = CC.weierstrass_decode_cases(cname)
        sweep = [c for c in cases if c.note == "sweep"]
        xs = CC.sweep_xs(cname)
        assert len(sweep) == 2 * len(xs)
        for x in [0, 15, p - 16, p - 1, p, p + 1, p + 16, (1 << 30) - 1, 1 << 30, 1 << 32, (1 << 32) + 1,
                  1 << (30 * 8), (1 << (32 * 7)) - 1]:
            assert x in xs, hex(x)
        if cname == "bls12_381":
            assert max(xs) == p + 16 and (1 << 360) in xs and (1 << 352) + 1 in xs
        else:
            assert max(xs) == (1 << 256) - 1 and (1 << 240) in xs and (1 << 224) + 1 in xs
        assert all(not c.ok for c, x in zip(sweep, [x for x in xs for _ in (0, 1)]) if x >= p)
        ok = [c for c in sweep if c.ok]
        assert ok and len(ok) < len(sweep)
        flags = collections.Counter((c.data[0] >> 5) & 1 if cname == "bls12_381" else c.data[0] & 1 for c in ok)
        assert flags[0] == flags[1] > 10
        assert len(ok) == len({c.point for c in ok})                  # the two flags give the two roots
        fl = [c for c in cases if c.note == "flags"]
        assert len(fl) == (24 if cname == "bls12_381" else 18) and any(c.ok for c in fl) and not all(c.ok for c in fl)
        assert any(c.ok and c.point is None for c in fl)              # the infinity encoding is among them


def test_census_of_the_hashed_keys():
    for cname in ("bls12_381", "secp256k1"):
        label, length, pts = CC.hashed_key_cases(cname)[0]
        assert length == 40 and len(pts) == 81
        assert sum(hp.ctr > 0 for hp in pts) >= 10
        assert sum(hp.flipped for hp in pts) >= 10 and sum(not hp.flipped for hp in pts) >= 10
    label, length, pts = CC.hashed_key_cases("ed25519")[0]
    maps = collections.Counter(m for hp in pts for m in hp.maps)
    assert set(maps) == set(itertools.product(OUTCOMES, BOOLS)) and len(pts) == 81, maps


def test_bls_half_points_sit_at_the_boundary():
    curve = P.BLS12_381
    p = curve["p"]
    half = (p - 1) // 2
    G = P.WeierstrassGroup(curve)
    cases = CC.bls_half_cases()
    bare = [c for c in cases if c.note[0] == "bare"]
    assert sum(1 for c in bare if c.note[1] < 0) >= 2 and sum(1 for c in bare if c.note[1] > 0) >= 2
    assert all(abs(c.note[1]) <= 8 and c.note[1] not in (0, 1) for c in bare)   # (p - 1) / 2 and (p + 1) / 2: not on the curve
    word = [c for c in cases if c.note[0] == "word"]
    assert len(word) >= 20 and len({c.note[1:3] for c in word}) >= 20
    # every word of the comparison: the step of word 0 is 1, its points are among the bare ones
    assert {c.note[1] for c in word} == set(range(1, 12))
    for c in word:
        _, i, sign, d = c.note
        assert c.point[1] == half + sign * (1 << (32 * i)) + d and 0 <= d <= 5
    for c, neg in zip(cases[0::2], cases[1::2]):
        assert neg.note == ("negative",) + c.note and neg.point == G.neg(c.point) and neg.above != c.above
    for c in cases:
        assert G.on_curve(c.point)
        assert c.above == (c.point[1] > half) == bool(c.data[0] & 0x20)
        assert c.data == P.compress_point(curve, c.point) and P.decompress_point(curve, c.data) == (True, c.point)
    assert not any(P.point_in_prime_subgroup(curve, G, c.point) for c in cases[:4])   # on the curve, outside G1


# ---- csrc/ristretto.hpp in a host build ---------------------------------------------------------------------------------
def _le(v):
    return v.to_bytes(32, "little").hex()


def _point(hx, hy):
    return (int.from_bytes(bytes.fromhex(hx), "little"), int.from_bytes(bytes.fromhex(hy), "little"))


def test_ristretto_host_build_equals_the_restatement(tmp_path):
    exe = str(tmp_path / ("bpp_ristretto_host_test" + ("_san" if SANITIZE else "")))
    subprocess.check_call(["g++", "-O1", "-std=c++17"] + SANITIZE +
                          ["-o", exe, os.path.join(ROOT, "tests", "host", "ristretto_host_test.cpp")])
    G = CC._edwards()
    dec, enc, uni = CC.rist_decode_cases(), CC.rist_encode_cases(), CC.uniform_cases()
    # rist_equal: every pair of representatives within a coset, and each coset against the next
    pairs = []
    for _, grp in itertools.groupby(enc, key=lambda c: c.coset):
        grp = [c.point for c in grp]
        pairs += [(a, b) for a in grp for b in grp]
    pairs += [(a.point, b.point) for a, b in zip(enc, enc[4:])]
    lines = ["dec " + c.data.hex() for c in dec] + ["enc %s %s" % (_le(c.point[0]), _le(c.point[1])) for c in enc] + \
            ["eq %s %s %s %s" % (_le(a[0]), _le(a[1]), _le(b[0]), _le(b[1])) for a, b in pairs] + ["uni " + b.hex() for b in uni]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, check=True, text=True).stdout.split("\n")
    assert len(out) == len(lines) + 1 and out[-1] == ""
    it = iter(out)
    for c in dec:
        got = next(it).split()
        assert got[0] == ("1" if c.point is not None else "0"), (c.data.hex(), c.reason)
        assert (_point(got[1], got[2]) if c.point is not None else None) == c.point and len(got) == (3 if c.point else 1)
    for c in enc:
        assert bytes.fromhex(next(it)) == c.data, (c.note, c.trace)
    for a, b in pairs:
        assert next(it) == ("1" if R.equal(a, b) else "0")
    assert sum(R.equal(a, b) for a, b in pairs) == 16 * (len(enc) // 4)
    for b in uni:
        got = next(it).split()
        want = R.from_uniform_bytes(b, G) or (0, 1)
        assert _point(got[0], got[1]) == want, b.hex()
    # the inputs this build exists for are in the list: a half at or above p, and bit 255 set
    ts = [int.from_bytes(b[32 * h:32 * h + 32], "little") for b in uni for h in range(2)]
    assert {t for t in ts if R.P <= t < 1 << 255} == set(range(R.P, 1 << 255)) and sum(t >> 255 for t in ts) >= 4
    assert {0, 1, R.P - 1} <= set(ts)
    # the derivation reduces where the decoder rejects: t and t - p give the same element
    fixed = uni[64][32:]
    for t in range(R.P, 1 << 255):
        above, below = t.to_bytes(32, "little") + fixed, (t - R.P).to_bytes(32, "little") + fixed
        assert R.from_uniform_bytes(above, G) == R.from_uniform_bytes(below, G)
