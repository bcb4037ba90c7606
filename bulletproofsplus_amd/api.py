"""Host-side mirror of the reference crate's public API for the hot path, over the C ABI.

Names, argument meaning and error behaviour follow the reference (paths relative to /root/reference/src):

  Arith.init()                        bls12_381/building_block/arith.rs:6-19
  MulVec                              bls12_381/building_block/mulvec.rs:7-53
  PublicKey(length) / .commitment     publickey.rs:13-52
  RangeProver / .commit               range/prover.rs:13-42
  RangeProof.prove / .verify          range/mod.rs:25-78
  WeightedInnerProductProof (fields)  weighted_inner_product_proof.rs:25-33
  ProofError                          errors.rs:14-50 (only VerificationError is ever constructed)

plus ``BatchVerifier``, the device-resident batch path the reference does not have.

Data is numpy ``uint64`` in the wire format of include/bpp_amd.h: scalars (..., 4), points (..., 2L+1).
Python ints are accepted for scalars.  Every call runs HIP kernels; nothing is computed on the CPU
beyond (de)serialisation.
"""

from __future__ import annotations

import contextlib
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import BLS12_381_G1, SECP256K1, ED25519, CURVE_IDS, BppError, check  # noqa: F401


AMOUNT64 = 0x100   # BPP_PROVE_AMOUNT64 (include/bpp_amd.h): commitments over the whole 64-bit amount
AMOUNTS_SEALED = 0x200   # BPP_FIND_AMOUNTS_SEALED: verify_find's amounts are one sealed amount per proof
SCAN_UNCONFIRMED = 3   # BPP_SCAN_UNCONFIRMED: a scanned proof with no candidate amount, or of more than one output


class ProofError(Exception):
    """reference src/errors.rs:14-50"""


class VerificationError(ProofError):
    """ProofError::VerificationError"""


def _ptr(a):
    """the one doorway from arrays to pointers (None stays None)"""
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _some(a):
    """_ptr, with None for an empty array as well as for an absent one"""
    return _ptr(a) if a is not None and len(a) else None


def _flat_bytes(x) -> np.ndarray:
    """bytes, or anything array-like, as one flat u8 array"""
    return np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else \
        np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)


def _flags(transcript=False, uncompressed=False, amount64=False, sealed=False) -> int:
    """the flag word of the serialized, prove, scan and find entries (include/bpp_amd.h)"""
    return (1 if transcript else 0) | (2 if uncompressed else 0) | (AMOUNT64 if amount64 else 0) | \
        (AMOUNTS_SEALED if sealed else 0)


def _index_arg(index, count, message: str):
    """None, or one u64 per item: RuntimeError(message) when there are not `count` of them (count None: any number)"""
    if index is None:
        return None
    idx = np.ascontiguousarray(np.asarray([int(x) for x in index], dtype=np.uint64))
    if count is not None and len(idx) != count:
        raise RuntimeError(message)
    return idx


def _amounts_arg(amounts, need=None, message: str = None, rows: bool = False) -> np.ndarray:
    """amounts below 2^64 as one flat u64 array -- one list, or (rows) one list per key flattened key-major;
    RuntimeError(message) when there are not `need` of them (need None: any number)"""
    vals = [[int(x) for x in row] for row in amounts] if rows else [int(x) for x in amounts]
    am = np.ascontiguousarray(np.asarray(vals, dtype=np.uint64).reshape(-1))
    if need is not None and len(am) != need:
        raise RuntimeError(message)
    return am


def _tags_arg(tags) -> np.ndarray:
    """view-tag bytes (bytes, or a sequence of ints) as one flat u8 array"""
    return _flat_bytes(tags) if isinstance(tags, (bytes, bytearray, memoryview)) else \
        np.ascontiguousarray(np.asarray([int(x) for x in tags], dtype=np.uint8).reshape(-1))


@contextlib.contextmanager
def _packed_keys(where: str, keys):
    """-> (the 32-byte keys packed into one u8 array, or None when there are none; their number).  The packed copy made
    here is wiped on every way out, as the C++ host twins wipe theirs (csrc/staging.hpp)."""
    keys = [bytes(k) for k in keys]
    if any(len(k) != 32 for k in keys):
        raise RuntimeError("%s: every key is 32 bytes" % where)
    kb = np.frombuffer(b"".join(keys), dtype=np.uint8).copy() if keys else None
    try:
        yield kb, len(keys)
    finally:
        if kb is not None:
            kb[:] = 0


def _hits(rec, found: int) -> list:
    """the find entries' 12-word records [key number, position, amount lo, hi, mask as 8 words], the first `found` that
    were written -> [(key_no, position, amount, mask)]"""
    return [(int(r[0]), int(r[1]), int(r[2]) | int(r[3]) << 32, wire_to_int(np.ascontiguousarray(r[4:]).view(np.uint64)))
            for r in rec[:found]]


def scalar_to_wire(x) -> np.ndarray:
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x, dtype=np.uint64).reshape(4)
    x = int(x)
    return np.array([(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def scalars_to_wire(xs) -> np.ndarray:
    if isinstance(xs, np.ndarray) and xs.dtype == np.uint64:
        return np.ascontiguousarray(xs).reshape(-1, 4)
    out = np.zeros((len(xs), 4), dtype=np.uint64)
    for i, x in enumerate(xs):
        out[i] = scalar_to_wire(x)
    return out


def wire_to_int(a) -> int:
    v = 0
    for i, w in enumerate(np.asarray(a, dtype=np.uint64).reshape(-1).tolist()):
        v |= int(w) << (64 * i)
    return v


class Arith:
    """One context per (curve, device); ``Arith.init()`` mirrors the reference's global one-time init."""

    _ctxs = {}

    def __init__(self, curve=BLS12_381_G1, device=0):
        if isinstance(curve, str):
            curve = CURVE_IDS[curve]
        self.curve = curve
        self.device = device
        self.L = _lib.FP_LIMBS[curve]
        self.PW = 2 * self.L + 1
        h = ctypes.c_void_p()
        check(_lib.lib().bpp_init(curve, device, ctypes.byref(h)), "bpp_init")
        self.handle = h

    @classmethod
    def init(cls, curve=BLS12_381_G1, device=0) -> "Arith":
        if isinstance(curve, str):
            curve = CURVE_IDS[curve]
        key = (curve, device)
        if key not in cls._ctxs:
            cls._ctxs[key] = cls(curve, device)
        return cls._ctxs[key]

    def set_verify_cache(self, on: bool):
        """the per-key small-table verifiers behind RangeProof.verify (include/bpp_amd.h, bpp_range_verify); on by default"""
        check(_lib.lib().bpp_set_verify_cache(self.handle, 1 if on else 0), "bpp_set_verify_cache")

    # Point::zero()
    def zero_point(self) -> np.ndarray:
        z = np.zeros(self.PW, dtype=np.uint64)
        z[2 * self.L] = 1
        return z

    def is_zero(self, p) -> bool:
        return int(np.asarray(p).reshape(-1)[2 * self.L]) != 0

    # Point * PrimeFieldElem, n independent pairs
    def scalar_mul(self, scalars, points) -> np.ndarray:
        sc = scalars_to_wire(scalars)
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, self.PW)
        if sc.shape[0] != pts.shape[0]:
            raise ValueError("scalar_mul: lengths must match")
        out = np.zeros((sc.shape[0], self.PW), dtype=np.uint64)
        check(_lib.lib().bpp_scalar_mul_batch(self.handle, _ptr(sc), _ptr(pts), sc.shape[0], _ptr(out)),
              "bpp_scalar_mul_batch")
        return out


class MulVec:
    """reference bls12_381/building_block/mulvec.rs: append scalars, append points, calculate()."""

    def __init__(self, arith: Arith):
        self.arith = arith
        self.scalars = []
        self.points = []

    def add_scalar(self, s):
        self.scalars.append(scalar_to_wire(s))

    def add_scalars(self, ss):
        for s in ss:
            self.add_scalar(s)

    def add_point(self, p):
        self.points.append(np.ascontiguousarray(p, dtype=np.uint64).reshape(self.arith.PW))

    def add_points(self, ps):
        for p in np.asarray(ps, dtype=np.uint64).reshape(-1, self.arith.PW):
            self.add_point(p)

    def calculate(self) -> np.ndarray:
        if len(self.scalars) != len(self.points):
            # the reference panics here (mulvec.rs:23-25)
            raise RuntimeError("mulvec: lengths of scalars and points must match")
        n = len(self.scalars)
        sc = np.stack(self.scalars) if n else np.zeros((0, 4), np.uint64)
        pts = np.stack(self.points) if n else np.zeros((0, self.arith.PW), np.uint64)
        out = np.zeros(self.arith.PW, dtype=np.uint64)
        check(_lib.lib().bpp_msm(self.arith.handle, _ptr(sc), _ptr(pts), n, _ptr(out)), "bpp_msm")
        return out


def msm_pippenger(arith: Arith, scalars, points, window_bits: int = 0) -> np.ndarray:
    """MulVec::calculate through the bucket-method pipeline (any n; window_bits 0 = chosen from n)."""
    sc = scalars_to_wire(scalars)
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, arith.PW)
    if sc.shape[0] != pts.shape[0]:
        raise RuntimeError("mulvec: lengths of scalars and points must match")
    out = np.zeros(arith.PW, dtype=np.uint64)
    check(_lib.lib().bpp_msm_pippenger(arith.handle, _ptr(sc), _ptr(pts), sc.shape[0], window_bits, _ptr(out)),
          "bpp_msm_pippenger")
    return out


def msm_workspace_bytes(arith: Arith, n: int, window_bits: int = 0) -> int:
    return _lib.lib().bpp_msm_workspace_bytes(arith.handle, n, window_bits)


def msm_device(arith: Arith, d_scalars: int, d_points: int, n: int, d_out: int, d_workspace: int, workspace_bytes: int,
               window_bits: int = 0, d_status: int = 0, stream: int = 0):
    """MulVec::calculate with every buffer in HBM (raw device pointers, e.g. torch tensors' data_ptr()), asynchronous
    on `stream`: d_scalars (n, 4) u64, d_points (n, PW) u64 wire points, d_out one wire point, d_status one u32."""
    check(_lib.lib().bpp_msm_device(arith.handle, d_scalars or None, d_points or None, n, window_bits, d_out,
                                    d_status or None, d_workspace, workspace_bytes, stream or None), "bpp_msm_device")


MSM_STAGES = ("sort", "chunks", "fold", "reduce", "final")


def msm_set_profiling(arith: Arith, on: bool):
    check(_lib.lib().bpp_msm_set_profiling(arith.handle, 1 if on else 0), "bpp_msm_set_profiling")


def msm_profile(arith: Arith):
    """-> ({stage: mean ms}, passes, shape dict of the last bpp_msm_device call), HIP events on the launch stream"""
    ms = (ctypes.c_float * 5)()
    passes = ctypes.c_size_t()
    sh = (ctypes.c_uint32 * 8)()
    check(_lib.lib().bpp_msm_profile(arith.handle, ms, ctypes.byref(passes), sh), "bpp_msm_profile")
    keys = ("n", "items", "windows", "narrow_bits", "wide_windows", "buckets", "chunk_entries", "window_bits")
    return {k: float(ms[i]) for i, k in enumerate(MSM_STAGES)}, passes.value, {k: int(sh[i]) for i, k in enumerate(keys)}


def msm_batch(arith: Arith, scalars, points, lens) -> np.ndarray:
    """`len(lens)` independent MulVecs in one launch."""
    sc = scalars_to_wire(scalars)
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, arith.PW)
    ln = np.ascontiguousarray(lens, dtype=np.uint32)
    if int(ln.sum()) != sc.shape[0] or sc.shape[0] != pts.shape[0]:
        raise RuntimeError("mulvec: lengths of scalars and points must match")
    out = np.zeros((len(ln), arith.PW), dtype=np.uint64)
    check(_lib.lib().bpp_msm_batch(arith.handle, _ptr(sc), _ptr(pts), _ptr(ln), len(ln), _ptr(out)), "bpp_msm_batch")
    return out


def wip_fold_round(arith: Arith, a, b, G, H, y_nhat, e):
    """One folding round of WeightedInnerProductProof::prove (wip.rs:147-164).  a, b: (len, 4) scalars; G, H: (len, PW)
    points.  Returns the folded (a, b, G, H) of length len / 2."""
    aw = np.ascontiguousarray(scalars_to_wire(a)).copy()
    bw = np.ascontiguousarray(scalars_to_wire(b)).copy()
    Gw = np.ascontiguousarray(G, dtype=np.uint64).reshape(-1, arith.PW).copy()
    Hw = np.ascontiguousarray(H, dtype=np.uint64).reshape(-1, arith.PW).copy()
    n = aw.shape[0]
    if not (bw.shape[0] == Gw.shape[0] == Hw.shape[0] == n):
        raise AssertionError("wip fold: vector lengths must match")          # wip.rs:60-67 asserts
    check(_lib.lib().bpp_wip_fold_round(arith.handle, _ptr(aw), _ptr(bw), _ptr(Gw), _ptr(Hw), n,
                                        _ptr(scalar_to_wire(y_nhat)), _ptr(scalar_to_wire(e))), "bpp_wip_fold_round")
    h = n // 2
    return aw[:h], bw[:h], Gw[:h], Hw[:h]


def compressed_bytes(arith: Arith) -> int:
    """bytes of one compressed point (48 BLS12-381 G1, 33 secp256k1 SEC1; 0 = not offered)"""
    return _lib.lib().bpp_point_compressed_bytes(arith.curve)


def compress_points(arith: Arith, points) -> np.ndarray:
    """wire points (n, PW) u64 -> (n, compressed_bytes) u8.  No reference counterpart (include/bpp_amd.h)."""
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, arith.PW)
    out = np.zeros((pts.shape[0], compressed_bytes(arith)), dtype=np.uint8)
    check(_lib.lib().bpp_points_compress(arith.handle, _ptr(pts), pts.shape[0], _ptr(out)), "bpp_points_compress")
    return out


def decompress_points(arith: Arith, data):
    """(n, compressed_bytes) u8 -> (wire points (n, PW) u64, ok (n,) u32: 0 valid / 1 malformed -> infinity)"""
    cb = compressed_bytes(arith)
    raw = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, cb)
    pts = np.zeros((raw.shape[0], arith.PW), dtype=np.uint64)
    ok = np.zeros(raw.shape[0], dtype=np.uint32)
    check(_lib.lib().bpp_points_decompress(arith.handle, _ptr(raw), raw.shape[0], _ptr(pts), _ptr(ok)),
          "bpp_points_decompress")
    return pts, ok


def proof_bytes(arith: Arith, n: int, m: int, version: int = 1) -> int:
    """bytes of one serialized proof (include/bpp_amd.h, "the container"); version 2 = uncompressed points"""
    return _lib.lib().bpp_proof_bytes_version(arith.curve, n, m, version)


def uncompressed_bytes(arith: Arith) -> int:
    """bytes of one uncompressed point (96 BLS12-381 G1, 65 secp256k1 SEC1; 0 = not offered)"""
    return _lib.lib().bpp_point_uncompressed_bytes(arith.curve)


def uncompressed_points(arith: Arith, points) -> np.ndarray:
    """wire points (n, PW) u64 -> (n, uncompressed_bytes) u8: the point encoding of container version 2"""
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, arith.PW)
    out = np.zeros((pts.shape[0], uncompressed_bytes(arith)), dtype=np.uint8)
    check(_lib.lib().bpp_points_uncompressed(arith.handle, _ptr(pts), pts.shape[0], _ptr(out)), "bpp_points_uncompressed")
    return out


def encode_proofs(arith: Arith, n: int, m: int, points, scalars, version: int = 1) -> np.ndarray:
    """points (count, 3+2k, PW), scalars (count, 3, 4) -> (count, proof_bytes) u8.  No reference counterpart."""
    k = (n * m).bit_length() - 1
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 3 + 2 * k, arith.PW)
    sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 3, 4)
    if sc.shape[0] != pts.shape[0]:
        raise RuntimeError("encode_proofs: one scalar triple per proof")
    out = np.zeros((pts.shape[0], proof_bytes(arith, n, m, version)), dtype=np.uint8)
    check(_lib.lib().bpp_proofs_encode_version(arith.handle, n, m, version, _ptr(pts), _ptr(sc), pts.shape[0], _ptr(out)),
          "bpp_proofs_encode_version")
    return out


def decode_proofs(arith: Arith, n: int, m: int, data):
    """(count, proof_bytes) u8 -> (points, scalars, status); status 0 valid / 2 FormatError"""
    k = (n * m).bit_length() - 1
    raw = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, proof_bytes(arith, n, m))
    count = raw.shape[0]
    pts = np.zeros((count, 3 + 2 * k, arith.PW), dtype=np.uint64)
    sc = np.zeros((count, 3, 4), dtype=np.uint64)
    st = np.zeros(count, dtype=np.uint32)
    check(_lib.lib().bpp_proofs_decode(arith.handle, n, m, _ptr(raw), count, _ptr(pts), _ptr(sc), _ptr(st)), "bpp_proofs_decode")
    return pts, sc, st


def proofs_scan(arith, n: int, data, version: int = 1) -> np.ndarray:
    """Frames a bare byte stream of concatenated containers (bpp_proofs_scan; host code, no device): -> m_i per container,
    (count,) u32.  arith: an Arith, a curve name or a curve id.  Raises BppError, naming the container and its byte
    offset, when the stream cannot be framed."""
    curve = getattr(arith, "curve", arith)
    if isinstance(curve, str):
        curve = CURVE_IDS[curve]
    raw = _flat_bytes(data)
    shortest = _lib.lib().bpp_proof_bytes_version(curve, n, 1, version)   # bounds the count
    ms = np.zeros(len(raw) // shortest if shortest else 0, dtype=np.uint32)
    count = ctypes.c_size_t(0)
    check(_lib.lib().bpp_proofs_scan(curve, n, version, _some(raw), len(raw), _some(ms), len(ms), ctypes.byref(count)),
          "bpp_proofs_scan")
    return ms[:count.value]


def mixed_groups(ms, group: int) -> np.ndarray:
    """The partition of the grouped check over a mixed batch (bpp_verifier_run_grouped_mixed; pure host code): the group
    number of every proof, in caller order.  The batch is gathered by aggregation size -- the proofs with ms[i] = 1 in caller
    order, then those with 2, 4, ... -- and group g holds the gathered positions [g * group, (g + 1) * group): a group may
    hold proofs of several sizes and the last one may be short.  `stats` of the call = (groups holding at least one proof the
    exact check rejects, the sizes of those groups)."""
    m = np.ascontiguousarray(ms, dtype=np.uint32).reshape(-1)
    if group < 2 or group & (group - 1):
        raise ValueError("group must be a power of two, at least 2")
    if len(m) and (m.min() == 0 or np.any(m & (m - 1))):
        raise ValueError("every ms[i] must be a power of two")
    pos = np.empty(len(m), dtype=np.int64)
    pos[np.argsort(m, kind="stable")] = np.arange(len(m))   # gathered position of caller i
    return pos // group


class FormatError(ProofError):
    """ProofError::FormatError (reference src/errors.rs:20): a serialized proof that does not parse"""


class PublicKey:
    """reference publickey.rs:13-52.  Fields g, h, G_vec, H_vec as in the reference."""

    def __init__(self, arith: Arith, length: int):
        self.arith = arith
        PW = arith.PW
        self.gh = np.zeros((2, PW), dtype=np.uint64)
        self.G_vec = np.zeros((max(length, 1), PW), dtype=np.uint64)
        self.H_vec = np.zeros((max(length, 1), PW), dtype=np.uint64)
        check(_lib.lib().bpp_pk_new(arith.handle, length, _ptr(self.gh), _ptr(self.G_vec), _ptr(self.H_vec)),
              "bpp_pk_new")
        self.G_vec = self.G_vec[:length]
        self.H_vec = self.H_vec[:length]

    @classmethod
    def new(cls, arith: Arith, length: int) -> "PublicKey":
        return cls(arith, length)

    @classmethod
    def hashed(cls, arith: Arith, length: int, label: bytes = b"") -> "PublicKey":
        """Generators hashed to the group from `label` (g stays the base point): what a deployment uses instead of the
        reference's test generators.  No reference counterpart (include/bpp_amd.h, bpp_pk_hashed)."""
        self = cls.__new__(cls)
        self.arith = arith
        PW = arith.PW
        self.gh = np.zeros((2, PW), dtype=np.uint64)
        G = np.zeros((max(length, 1), PW), dtype=np.uint64)
        H = np.zeros((max(length, 1), PW), dtype=np.uint64)
        check(_lib.lib().bpp_pk_hashed(arith.handle, bytes(label), len(label), length, _ptr(self.gh), _ptr(G), _ptr(H)),
              "bpp_pk_hashed")
        self.G_vec, self.H_vec = G[:length], H[:length]
        return self

    @classmethod
    def from_points(cls, arith: Arith, gh, G_vec, H_vec) -> "PublicKey":
        """An arbitrary generator set (the reference only has `new`; used for the 'hard' distribution)."""
        self = cls.__new__(cls)
        self.arith = arith
        self.gh = np.ascontiguousarray(gh, dtype=np.uint64).reshape(2, arith.PW)
        self.G_vec = np.ascontiguousarray(G_vec, dtype=np.uint64).reshape(-1, arith.PW)
        self.H_vec = np.ascontiguousarray(H_vec, dtype=np.uint64).reshape(-1, arith.PW)
        return self

    @property
    def g(self):
        return self.gh[0]

    @property
    def h(self):
        return self.gh[1]

    def commitment(self, v, gamma) -> np.ndarray:
        """g * v + h * gamma (publickey.rs:50-52); v, gamma scalars."""
        mv = MulVec(self.arith)
        mv.add_scalar(v)
        mv.add_scalar(gamma)
        mv.add_point(self.g)
        mv.add_point(self.h)
        return mv.calculate()


class RangeProver:
    """reference range/prover.rs:13-42."""

    def __init__(self):
        self.v_vec = []
        self.gamma_vec = []
        self.commitment_vec = []

    @classmethod
    def new(cls):
        return cls()

    def commit(self, pk: PublicKey, v: int, gamma, amount64: bool = False):
        """range/prover.rs:28-42.  amount64=False keeps the `v as i32` of prover.rs:37; amount64=True commits the whole
        64-bit amount, v g + gamma h (a two-term MulVec), what a proof of an amount of 2^31 or more verifies against."""
        g = scalar_to_wire(gamma)
        if amount64:
            if not 0 <= int(v) < 1 << 64:
                raise ValueError("amount64: 0 <= v < 2^64")
            out = pk.commitment(int(v), g)
        else:
            out = np.zeros(pk.arith.PW, dtype=np.uint64)
            check(_lib.lib().bpp_commit(pk.arith.handle, _ptr(pk.gh), ctypes.c_uint64(v), _ptr(g), _ptr(out)), "bpp_commit")
        self.v_vec.append(int(v))
        self.gamma_vec.append(g)
        self.commitment_vec.append(out)


class RangeVerifier:
    """The verifier-side holder of the commitments.  It exists only in the reference's (stale) README
    (README.md:47-55: ``RangeVerifier::new()``, ``allocate(&prover.commitment_vec)``, ``proof.verify(.., &verifier)``);
    the code takes the commitment slice directly (range/mod.rs:57-62).  ``RangeProof.verify`` accepts either."""

    def __init__(self):
        self.commitment_vec = []

    @classmethod
    def new(cls):
        return cls()

    def allocate(self, commitment_vec):
        self.commitment_vec = [np.ascontiguousarray(c, dtype=np.uint64) for c in commitment_vec]


# the scalar-field orders r (group orders of the three instantiations)
FR_ORDER = {
    BLS12_381_G1: 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
    _lib.SECP256K1: 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141,
    _lib.ED25519: (1 << 252) + 27742317777372353535851937790883648493,
}


def _scalar_int(x) -> int:
    return wire_to_int(x) if isinstance(x, np.ndarray) else int(x)


def _wip_y(arith, power_of_y_vec, length: int) -> int:
    """the y of a power_of_y_vec = [y, y^2, .., y^len] (exp_iter_type2), ValueError for anything else: the reference's
    verify reads only the first entry (wip.rs:252) and rebuilds the rest, which is what the engine does"""
    r = FR_ORDER[arith.curve]
    pw = [_scalar_int(x) % r for x in power_of_y_vec]
    if len(pw) != length:
        raise ValueError("power_of_y_vec must hold one power per generator")
    y, cur = pw[0], 1
    for x in pw:
        cur = cur * y % r
        if x != cur:
            raise ValueError("power_of_y_vec must be [y, y^2, .., y^len]")
    return y


class WeightedInnerProductProof:
    """reference weighted_inner_product_proof.rs:25-33, with prove (:36-227) and verify (:238-328) on the engine's WIP
    seam (include/bpp_amd.h, bpp_wip_prove_batch / bpp_wip_verify_batch)."""

    def __init__(self, L_vec, R_vec, A, B, r_prime, s_prime, d_prime):
        self.L_vec, self.R_vec, self.A, self.B = L_vec, R_vec, A, B
        self.r_prime, self.s_prime, self.d_prime = r_prime, s_prime, d_prime

    @staticmethod
    def _engine(pk, engine):
        length = len(pk.G_vec)
        if engine is None:   # a small engine of its own: only n m = len counts (n <= 64)
            n = min(length, 64)
            return BatchVerifier(pk, n, length // n, window_bits=4), True
        if engine.n * engine.m != length:
            raise AssertionError("the engine's key must hold len generators")
        return engine, False

    @classmethod
    def prove(cls, pk, a_vec, b_vec, power_of_y_vec, gamma, commitment=None, engine=None) -> "WeightedInnerProductProof":
        """WeightedInnerProductProof::prove with the reference's argument list (`commitment` is dead there, wip.rs:57, and
        is ignored here); the reference's literal challenges and blinding"""
        length = len(pk.G_vec)
        if len(pk.H_vec) != length or len(a_vec) != length or len(b_vec) != length or length & (length - 1) or not length:
            raise AssertionError("a_vec, b_vec and the key must have the same power-of-two length")   # wip.rs:60-67
        y = _wip_y(pk.arith, power_of_y_vec, length)
        eng, own = cls._engine(pk, engine)
        try:
            pts, sc, _ = eng.wip_prove_batch([a_vec], [b_vec], [y], [gamma])
        finally:
            if own:
                eng.close()
        k = eng.k
        p = pts[0]
        return cls(p[3:3 + k], p[3 + k:3 + 2 * k], p[1], p[2], sc[0, 0], sc[0, 1], sc[0, 2])

    def verify(self, pk, power_of_y_vec, G_exp, H_exp, g_exp, V_exp, A_prime, V, engine=None) -> None:
        """WeightedInnerProductProof::verify with the reference's argument list (the four *_exp_of_commitment arguments,
        wip.rs:238-247).  Returns None for Ok(()); raises VerificationError."""
        length = len(pk.G_vec)
        if (1 << len(self.L_vec)) != length or len(self.R_vec) != len(self.L_vec):
            raise VerificationError("VerificationError")                                              # wip.rs:335-337
        if len(G_exp) != length or len(H_exp) != length or len(V_exp) != len(V):
            raise AssertionError("statement exponents must match the key and V")                      # mulvec.rs:23-25
        y = _wip_y(pk.arith, power_of_y_vec, length)
        eng, own = self._engine(pk, engine)
        try:
            PW = pk.arith.PW
            rec = np.concatenate([np.asarray(A_prime, dtype=np.uint64).reshape(1, PW), np.stack([self.A, self.B]),
                                  np.asarray(self.L_vec, dtype=np.uint64).reshape(-1, PW),
                                  np.asarray(self.R_vec, dtype=np.uint64).reshape(-1, PW),
                                  np.asarray(V, dtype=np.uint64).reshape(-1, PW)]).astype(np.uint64)
            sc = np.stack([scalar_to_wire(self.r_prime), scalar_to_wire(self.s_prime), scalar_to_wire(self.d_prime)])
            stm = list(G_exp) + list(H_exp) + [g_exp] + list(V_exp)
            ok = eng.wip_verify_batch(rec[None], sc[None], [y], [stm], nv=len(V))
        finally:
            if own:
                eng.close()
        if int(ok[0]) != 0:
            raise VerificationError("VerificationError")


class RangeProof:
    """reference range/mod.rs:25-78: struct RangeProof { A, proof }."""

    def __init__(self, A, proof: WeightedInnerProductProof):
        self.A = A
        self.proof = proof

    # wire record used by the C ABI: points [A, wip.A, wip.B, L.., R..], scalars [r', s', d']
    def points_wire(self) -> np.ndarray:
        p = self.proof
        return np.concatenate([np.stack([self.A, p.A, p.B]), np.asarray(p.L_vec), np.asarray(p.R_vec)]).astype(np.uint64)

    def scalars_wire(self) -> np.ndarray:
        p = self.proof
        return np.stack([scalar_to_wire(p.r_prime), scalar_to_wire(p.s_prime), scalar_to_wire(p.d_prime)])

    @classmethod
    def from_wire(cls, points, scalars) -> "RangeProof":
        points = np.asarray(points, dtype=np.uint64)
        k = (points.shape[0] - 3) // 2
        sc = np.asarray(scalars, dtype=np.uint64).reshape(3, 4)
        return cls(points[0], WeightedInnerProductProof(points[3:3 + k], points[3 + k:3 + 2 * k], points[1], points[2],
                                                        sc[0], sc[1], sc[2]))

    @classmethod
    def prove(cls, pk: PublicKey, n: int, prover: RangeProver) -> "RangeProof":
        a = pk.arith
        m = len(prover.v_vec)
        mn = n * m
        if m == 0 or mn & (mn - 1):
            raise AssertionError("n * m must be a power of two")      # wip.rs:67 assert
        if len(pk.G_vec) != mn or len(pk.H_vec) != mn:
            raise AssertionError("pk must hold n*m generators")       # range/mod.rs:90-91,252-253 assert_eq
        k = mn.bit_length() - 1
        v = np.array(prover.v_vec, dtype=np.uint64)
        gm = np.stack(prover.gamma_vec)
        V = np.stack(prover.commitment_vec)
        pts = np.zeros((3 + 2 * k, a.PW), dtype=np.uint64)
        sc = np.zeros((3, 4), dtype=np.uint64)
        G = np.ascontiguousarray(pk.G_vec)
        H = np.ascontiguousarray(pk.H_vec)
        check(_lib.lib().bpp_range_prove(a.handle, _ptr(pk.gh), _ptr(G), _ptr(H), n, m, _ptr(v), _ptr(gm), _ptr(V),
                                         _ptr(pts), _ptr(sc)), "bpp_range_prove")
        return cls.from_wire(pts, sc)

    def verify(self, pk: PublicKey, n: int, commitment_vec) -> None:
        """Returns None for Ok(()); raises VerificationError for Err(ProofError::VerificationError)."""
        a = pk.arith
        if isinstance(commitment_vec, RangeVerifier):   # the README's calling convention
            commitment_vec = commitment_vec.commitment_vec
        V = np.ascontiguousarray(np.asarray(commitment_vec, dtype=np.uint64).reshape(-1, a.PW))
        m = V.shape[0]
        if len(pk.G_vec) != n * m or len(pk.H_vec) != n * m:
            # the reference indexes pk.G_vec / H_vec with bounds-checked slices and panics (mulvec.rs:23-25)
            raise AssertionError("pk must hold n*m generators")
        pts = np.ascontiguousarray(self.points_wire())
        sc = np.ascontiguousarray(self.scalars_wire())
        k = (pts.shape[0] - 3) // 2
        G = np.ascontiguousarray(pk.G_vec)
        H = np.ascontiguousarray(pk.H_vec)
        rc = check(_lib.lib().bpp_range_verify(a.handle, _ptr(pk.gh), _ptr(G), _ptr(H), n, m, _ptr(pts), k, _ptr(sc),
                                               _ptr(V)), "bpp_range_verify")
        if rc != 0:
            raise VerificationError("VerificationError")


STAGES = ("from_wire", "verify_scalars", "fixed_msm", "var_msm", "finalize")


def _weight_key_arg(weight_key, d_weights):
    """The weighted checks' key argument: None when the weights come from d_weights, else 32 bytes (weight_key None = drawn
    here from os.urandom, fresh per call)."""
    if d_weights:
        return None
    if weight_key is None:
        weight_key = os.urandom(32)
    key = bytes(weight_key)
    if len(key) != 32:
        raise ValueError("weight_key must be 32 bytes")
    return key


def _prover_key(blind_key, transcript):
    """the provers' blinding key: None, or 32 bytes under the transcript"""
    if blind_key is not None and (not transcript or len(blind_key) != 32):
        raise ValueError("blind_key: 32 bytes, transcript mode only")


class _Shapes:
    """The shape arithmetic of an engine of capacity (n, m) over `arith`, and the front of the calls that take a block of
    proofs of mixed aggregation sizes: what BatchVerifier and VerifierPool share.  Proof i has shape (n, ms[i]), ms[i] a
    power of two <= m; an m_i the engine does not take is never an error here -- the checks that need the shapes are
    skipped and the library reports it (BPP_E_ARG naming the proof)."""

    def _ms(self, ms) -> np.ndarray:
        return np.ascontiguousarray(ms, dtype=np.uint32).reshape(-1)

    def _taken(self, ms) -> bool:
        return all(0 < int(x) <= self.m and not int(x) & (int(x) - 1) for x in ms)

    def _rounds(self, m_i: int) -> int:
        """k = log2(n m_i), the folding rounds of a proof of shape (n, m_i)"""
        return (self.n * m_i).bit_length() - 1

    def mixed_points(self, m_i: int) -> int:
        """wire points of a proof record of shape (n, m_i): 3 + 2 log2(n m_i) + m_i"""
        return 3 + 2 * self._rounds(m_i) + m_i

    def _wire_records(self, records) -> np.ndarray:
        """a list of per-proof records, or one packed array -> the packed (points, PW) array"""
        PW = self.arith.PW
        if not isinstance(records, (list, tuple)):
            pts = np.asarray(records, dtype=np.uint64).reshape(-1, PW)
        elif len(records):
            pts = np.concatenate([np.asarray(r, dtype=np.uint64).reshape(-1, PW) for r in records])
        else:
            pts = np.zeros((0, PW), dtype=np.uint64)
        return np.ascontiguousarray(pts)

    def _block(self, where: str, proofs, commitments, ms, uncompressed: bool):
        """The front of every call that takes containers back to back and ms[i] encoded commitments per proof:
        -> (raw u8, cm u8, ms u32, count), ms framed from the stream (proofs_scan) when None.  RuntimeError, prefixed
        with `where`, when the byte counts are not the ones the shapes need."""
        raw, cm = _flat_bytes(proofs), _flat_bytes(commitments)
        version = 2 if uncompressed else 1
        m = proofs_scan(self.arith, self.n, raw, version) if ms is None else self._ms(ms)
        if self._taken(m):
            need = sum(proof_bytes(self.arith, self.n, int(x), version) for x in m)
            if len(raw) != need:
                raise RuntimeError("%s: %d bytes of proofs, the shapes in ms need %d" % (where, len(raw), need))
            if len(cm) != int(m.sum()) * (uncompressed_bytes(self.arith) if uncompressed else compressed_bytes(self.arith)):
                raise RuntimeError("%s: ms[i] commitments per proof" % where)
        return raw, cm, m, len(m)


class BatchVerifier(_Shapes):
    """Device-resident batch verification of independent proofs for one (pk, n, m).

    ``verify_wire`` takes host arrays; ``run_device`` takes raw device pointers (e.g. torch tensors'
    ``data_ptr()``) and is the call the benchmark times."""

    def __init__(self, pk: PublicKey, n: int, m: int, window_bits: int = 13):
        self.arith = pk.arith
        self.n, self.m = n, m
        if len(pk.G_vec) != n * m or len(pk.H_vec) != n * m:
            raise AssertionError("pk must hold n*m generators")       # range/mod.rs:90-91,252-253 assert_eq
        h = ctypes.c_void_p()
        G = np.ascontiguousarray(pk.G_vec)
        H = np.ascontiguousarray(pk.H_vec)
        check(_lib.lib().bpp_verifier_create(pk.arith.handle, _ptr(pk.gh), _ptr(G), _ptr(H), n, m, window_bits,
                                             ctypes.byref(h)), "bpp_verifier_create")
        self._adopt(h)

    def _adopt(self, handle):
        self.handle = handle
        self.msm_len = _lib.lib().bpp_verifier_msm_len(handle)
        self.table_bytes = _lib.lib().bpp_verifier_table_bytes(handle)
        self.k = self._rounds(self.m)
        self.points_per_proof = self.mixed_points(self.m)

    @classmethod
    def _borrowed(cls, arith: Arith, handle, n: int, m: int, owner) -> "BatchVerifier":
        """a verifier that belongs to `owner` (a VerifierPool's shard): close() leaves it alone"""
        v = cls.__new__(cls)
        v.arith, v.n, v.m, v._owner = arith, n, m, owner
        v._adopt(handle)
        return v

    def close(self):
        if self.handle and getattr(self, "_owner", None) is None:
            _lib.lib().bpp_verifier_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace_bytes(self, count: int) -> int:
        return _lib.lib().bpp_verifier_workspace_bytes(self.handle, count)

    def verify_wire(self, points, scalars) -> np.ndarray:
        """points (count, 3+2k+m, PW) [A, wip.A, wip.B, L.., R.., V..], scalars (count, 3, 4) -> ok (count,) u32"""
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, self.points_per_proof, self.arith.PW)
        sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 3, 4)
        count = pts.shape[0]
        if sc.shape[0] != count:
            raise RuntimeError("verify_wire: one scalar triple per proof record")
        ok = np.zeros(count, dtype=np.uint32)
        check(_lib.lib().bpp_range_verify_batch(self.handle, _ptr(pts), _ptr(sc), count, _ptr(ok)),
              "bpp_range_verify_batch")
        return ok

    def verify_compressed(self, records, scalars) -> np.ndarray:
        """records (count, 3+2k+m, compressed_bytes) u8 in the order of verify_wire, scalars (count, 3, 4) -> ok"""
        cb = compressed_bytes(self.arith)
        rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, self.points_per_proof, cb)
        sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 3, 4)
        count = rec.shape[0]
        if sc.shape[0] != count:
            raise RuntimeError("verify_compressed: one scalar triple per proof record")
        ok = np.zeros(count, dtype=np.uint32)
        check(_lib.lib().bpp_range_verify_batch_compressed(self.handle, _ptr(rec), _ptr(sc), count, _ptr(ok)),
              "bpp_range_verify_batch_compressed")
        return ok

    def verify_serialized(self, proofs, commitments, transcript: bool = False, uncompressed: bool = False) -> np.ndarray:
        """proofs (count, proof_bytes) u8, commitments (count, m, compressed_bytes) u8 -> status (count,) u32:
        0 Ok / 1 VerificationError / 2 FormatError.  uncompressed: container version 2 (and uncompressed commitments)"""
        pb = proof_bytes(self.arith, self.n, self.m, 2 if uncompressed else 1)
        raw = np.ascontiguousarray(proofs, dtype=np.uint8).reshape(-1, pb)
        cm = np.ascontiguousarray(commitments, dtype=np.uint8).reshape(
            -1, self.m, uncompressed_bytes(self.arith) if uncompressed else compressed_bytes(self.arith))
        if cm.shape[0] != raw.shape[0]:
            raise RuntimeError("verify_serialized: m commitments per proof")
        ok = np.zeros(raw.shape[0], dtype=np.uint32)
        check(_lib.lib().bpp_range_verify_batch_serialized(self.handle, _ptr(raw), _ptr(cm), raw.shape[0],
                                                           _flags(transcript, uncompressed), _ptr(ok)),
              "bpp_range_verify_batch_serialized")
        return ok

    def serialized_workspace_bytes(self, count: int) -> int:
        return _lib.lib().bpp_verifier_serialized_workspace_bytes(self.handle, count)

    def verify_serialized_device(self, d_proofs: int, d_commitments: int, count: int, d_ok: int, d_workspace: int,
                                 workspace_bytes: int, stream: int = 0, transcript: bool = False, uncompressed: bool = False):
        """verify_serialized with every buffer in HBM (raw device pointers), asynchronous on `stream`: containers and
        compressed (version 2: uncompressed) commitments in, per-proof status words (0 / 1 / 2) out"""
        check(_lib.lib().bpp_range_verify_batch_serialized_device(self.handle, d_proofs, d_commitments, count,
                                                                  _flags(transcript, uncompressed), d_ok, d_workspace,
                                                                  workspace_bytes, stream or None),
              "bpp_range_verify_batch_serialized_device")

    def serialized_grouped_workspace_bytes(self, count: int, group: int = 32) -> int:
        return _lib.lib().bpp_verifier_serialized_grouped_workspace_bytes(self.handle, count, group)

    def verify_serialized_grouped_device(self, d_proofs: int, d_commitments: int, count: int, d_ok: int, d_workspace: int,
                                         workspace_bytes: int, weight_key: bytes = None, index_base: int = 0, group: int = 32,
                                         stream: int = 0, transcript: bool = False, uncompressed: bool = False):
        """verify_serialized_device with the grouped check behind the decoder (include/bpp_amd.h): the same status words at the
        grouped check's price when (nearly) every proof is valid.  weight_key: 32 secret bytes, None = os.urandom(32).
        Synchronises the stream.  -> (groups that failed, proofs re-verified exactly)"""
        stats = (ctypes.c_uint64 * 2)()
        check(_lib.lib().bpp_range_verify_batch_serialized_grouped_device(
            self.handle, d_proofs, d_commitments, count, _flags(transcript, uncompressed), _weight_key_arg(weight_key, 0),
            ctypes.c_uint64(index_base), group, d_ok, stats, d_workspace, workspace_bytes, stream or None),
            "bpp_range_verify_batch_serialized_grouped_device")
        return int(stats[0]), int(stats[1])

    def run_device(self, d_points: int, d_scalars: int, count: int, d_ok: int, d_workspace: int, workspace_bytes: int,
                   stream: int = 0, d_challenges: int = 0, d_out_scalars: int = 0, d_out_result: int = 0):
        check(_lib.lib().bpp_verifier_run(self.handle, d_points, d_scalars, count, d_challenges or None, d_ok,
                                          d_workspace, workspace_bytes, d_out_scalars or None, d_out_result or None,
                                          stream or None), "bpp_verifier_run")

    def graph_capture(self, d_points: int, d_scalars: int, count: int, d_ok: int, d_workspace: int, workspace_bytes: int,
                      d_challenges: int = 0) -> PassGraph:
        h = ctypes.c_void_p()
        check(_lib.lib().bpp_verifier_graph_capture(self.handle, d_points, d_scalars, count, d_challenges or None, d_ok,
                                                    d_workspace, workspace_bytes, ctypes.byref(h)),
              "bpp_verifier_graph_capture")
        return PassGraph(h)

    def set_subgroup_check(self, on: bool):
        """wire points outside the prime-order subgroup count as invalid points (include/bpp_amd.h); off by default"""
        check(_lib.lib().bpp_verifier_set_subgroup_check(self.handle, 1 if on else 0), "bpp_verifier_set_subgroup_check")

    def set_profiling(self, on: bool):
        check(_lib.lib().bpp_verifier_set_profiling(self.handle, 1 if on else 0), "bpp_verifier_set_profiling")

    def profile(self):
        """-> ({stage: mean ms}, passes, blocks_per_proof of k_fixed_msm), HIP events on the launch stream"""
        ms = (ctypes.c_float * 5)()
        passes = ctypes.c_size_t()
        bpp_ = ctypes.c_uint()
        check(_lib.lib().bpp_verifier_profile(self.handle, ms, ctypes.byref(passes), ctypes.byref(bpp_)),
              "bpp_verifier_profile")
        return {k: float(ms[i]) for i, k in enumerate(STAGES)}, passes.value, bpp_.value

    def partial_bytes(self) -> int:
        return _lib.lib().bpp_verifier_partial_bytes(self.handle)

    def combined_workspace_bytes(self, count: int) -> int:
        return _lib.lib().bpp_verifier_combined_workspace_bytes(self.handle, count)

    def run_combined_device(self, d_points: int, d_scalars: int, count: int, weight_key, index_base: int,
                            d_out_partial: int, d_ok: int, d_workspace: int, workspace_bytes: int, stream: int = 0,
                            d_challenges: int = 0, d_weights: int = 0):
        """Combined batch check (NOT the reference's per-proof semantics, see include/bpp_amd.h): one weighted
        sum of the batch's verification MulVecs.  d_ok[0] == 0 iff it is the identity.
        weight_key: 32 secret bytes (None = drawn here from os.urandom, fresh per call) expanded on the device by a
        SHA-256 PRF over the global proof index index_base + p; or d_weights: count x 16 bytes on the device."""
        check(_lib.lib().bpp_verifier_run_combined(self.handle, d_points, d_scalars, count, d_challenges or None,
                                                   _weight_key_arg(weight_key, d_weights), ctypes.c_uint64(index_base),
                                                   d_weights or None, d_out_partial, d_ok, d_workspace, workspace_bytes,
                                                   stream or None),
              "bpp_verifier_run_combined")

    def grouped_workspace_bytes(self, count: int, group: int = 32) -> int:
        return _lib.lib().bpp_verifier_grouped_workspace_bytes(self.handle, count, group)

    def run_grouped_device(self, d_points: int, d_scalars: int, count: int, weight_key, index_base: int,
                           d_out_verdicts: int, d_workspace: int, workspace_bytes: int, group: int = 32,
                           stream: int = 0, d_challenges: int = 0, d_weights: int = 0):
        """Per-proof verdicts (the vector run_device writes) from one weighted check per group of `group` neighbouring proofs
        and an exact pass over the proofs of the groups that fail (include/bpp_amd.h "grouped check"; an engine mode, not a
        reference path).  weight_key / d_weights as for run_combined_device.  Synchronises the stream.
        Returns (groups that failed, proofs re-verified exactly)."""
        stats = (ctypes.c_uint64 * 2)()
        check(_lib.lib().bpp_verifier_run_grouped(self.handle, d_points, d_scalars, count, d_challenges or None,
                                                  _weight_key_arg(weight_key, d_weights), ctypes.c_uint64(index_base),
                                                  d_weights or None, group, d_out_verdicts, stats, d_workspace,
                                                  workspace_bytes, stream or None),
              "bpp_verifier_run_grouped")
        return int(stats[0]), int(stats[1])

    def grouped_begin_device(self, d_points: int, d_scalars: int, count: int, weight_key, index_base: int,
                             d_out_verdicts: int, d_workspace: int, workspace_bytes: int, group: int = 32, stream: int = 0,
                             d_challenges: int = 0, d_weights: int = 0):
        """First half of run_grouped_device: enqueues the weighted checks of the groups and returns (nothing synchronises)."""
        check(_lib.lib().bpp_verifier_grouped_begin(self.handle, d_points, d_scalars, count, d_challenges or None,
                                                    _weight_key_arg(weight_key, d_weights), ctypes.c_uint64(index_base),
                                                    d_weights or None, group, d_out_verdicts, d_workspace, workspace_bytes,
                                                    stream or None), "bpp_verifier_grouped_begin")

    def grouped_finish_device(self, d_points: int, d_scalars: int, count: int, d_out_verdicts: int, d_workspace: int,
                              workspace_bytes: int, group: int = 32, stream: int = 0, d_challenges: int = 0):
        """Second half: same buffers, count, group and stream as the begin it completes; synchronises the stream.
        -> (groups that failed, proofs re-verified exactly)"""
        stats = (ctypes.c_uint64 * 2)()
        check(_lib.lib().bpp_verifier_grouped_finish(self.handle, d_points, d_scalars, count, d_challenges or None, group,
                                                     d_out_verdicts, stats, d_workspace, workspace_bytes, stream or None),
              "bpp_verifier_grouped_finish")
        return int(stats[0]), int(stats[1])

    def derive_challenges_device(self, d_points: int, count: int, d_challenges: int, stream: int = 0):
        """Fiat-Shamir challenges [y, z, e, e_1..e_k] of every proof record of a resident batch (csrc/transcript.hpp),
        in the layout run_device takes as d_challenges.  The reference has no transcript: parity unpinned."""
        check(_lib.lib().bpp_verifier_derive_challenges(self.handle, d_points, count, d_challenges, stream or None),
              "bpp_verifier_derive_challenges")

    # ---- mixed batches: proof i of shape (n, ms[i]), ms[i] a power of two <= m (include/bpp_amd.h; _Shapes) ----
    def mixed_workspace_bytes(self, ms) -> int:
        """bytes of device workspace run_mixed_device / derive_challenges_mixed_device need (0: an m_i is not taken)"""
        m = self._ms(ms)
        return _lib.lib().bpp_verifier_mixed_workspace_bytes(self.handle, _ptr(m), len(m))

    def run_mixed_device(self, d_points: int, d_scalars: int, ms, d_ok: int, d_workspace: int, workspace_bytes: int,
                         stream: int = 0, d_challenges: int = 0, d_out_result: int = 0):
        """RangeProof::verify(proof_i, PublicKey::new(n ms[i]), n, V_i) for every proof of a resident batch: the verdict
        against the prefix key of the proof's own shape.  d_points: the packed records (mixed_points(ms[i]) wire points
        each, caller order); ms: host list.  Blocks while it uploads the per-proof index, the rest is on `stream`."""
        m = self._ms(ms)
        check(_lib.lib().bpp_verifier_run_mixed(self.handle, d_points, d_scalars, _ptr(m), len(m), d_challenges or None,
                                                d_ok, d_workspace, workspace_bytes, d_out_result or None, stream or None),
              "bpp_verifier_run_mixed")

    def derive_challenges_mixed_device(self, d_points: int, ms, d_challenges: int, d_workspace: int,
                                       workspace_bytes: int, stream: int = 0):
        """Fiat-Shamir challenges of a mixed batch, 3 + log2(n ms[i]) scalars per proof packed in caller order (the
        layout run_mixed_device takes); each transcript starts from the prefix key of the proof's own shape"""
        m = self._ms(ms)
        check(_lib.lib().bpp_verifier_derive_challenges_mixed(self.handle, d_points, _ptr(m), len(m), d_challenges,
                                                              d_workspace, workspace_bytes, stream or None),
              "bpp_verifier_derive_challenges_mixed")

    def verify_wire_mixed(self, records, scalars, ms) -> np.ndarray:
        """records: a list of per-proof (mixed_points(ms[i]), PW) arrays or one packed array; scalars (count, 3, 4);
        ms: m_i per proof -> ok (count,) u32 (bpp_range_verify_batch_mixed)"""
        m = self._ms(ms)
        count = len(m)
        taken = self._taken(m)
        need = sum(self.mixed_points(int(x)) for x in m) if taken else None
        if isinstance(records, (list, tuple)):
            if len(records) != count:
                raise RuntimeError("verify_wire_mixed: one record per entry of ms")
            for i, (r, x) in enumerate(zip(records, m)):
                if taken and np.asarray(r).reshape(-1, self.arith.PW).shape[0] != self.mixed_points(int(x)):
                    raise RuntimeError("verify_wire_mixed: record %d does not hold %d points" % (i, self.mixed_points(int(x))))
        pts = self._wire_records(records)
        if need is not None and pts.shape[0] != need:
            raise RuntimeError("verify_wire_mixed: %d wire points, the shapes in ms need %d" % (pts.shape[0], need))
        sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 3, 4)
        if sc.shape[0] != count:
            raise RuntimeError("verify_wire_mixed: one scalar triple per proof record")
        ok = np.zeros(count, dtype=np.uint32)
        check(_lib.lib().bpp_range_verify_batch_mixed(self.handle, _ptr(pts), _ptr(sc), _ptr(m), count, _ptr(ok)),
              "bpp_range_verify_batch_mixed")
        return ok

    # ---- serialized proofs of mixed aggregation sizes: bytes in, one status per proof out (include/bpp_amd.h) ----
    def serialized_mixed_workspace_bytes(self, ms) -> int:
        """bytes of device workspace verify_serialized_mixed_device needs (0: an m_i is not taken)"""
        m = self._ms(ms)
        return _lib.lib().bpp_verifier_serialized_mixed_workspace_bytes(self.handle, _ptr(m), len(m))

    def verify_serialized_mixed_device(self, d_proofs: int, d_commitments: int, ms, d_ok: int, d_workspace: int,
                                       workspace_bytes: int, stream: int = 0, transcript: bool = False,
                                       uncompressed: bool = False):
        """verify_serialized_device for a resident block of containers of mixed aggregation sizes: container i of
        proof_bytes(arith, n, ms[i]) bytes, packed back to back in caller order, and ms[i] encoded commitments per proof,
        packed likewise; ms: host list.  d_ok[i] = 0 / 1 / 2, the verdict against the prefix key of the proof's own shape.
        Blocks while it uploads the per-proof index, the rest is on `stream`."""
        m = self._ms(ms)
        check(_lib.lib().bpp_range_verify_batch_serialized_mixed_device(
            self.handle, d_proofs, d_commitments, _ptr(m), len(m), _flags(transcript, uncompressed),
            d_ok, d_workspace, workspace_bytes, stream or None), "bpp_range_verify_batch_serialized_mixed_device")

    def verify_serialized_mixed(self, proofs, commitments, ms=None, transcript: bool = False,
                                uncompressed: bool = False) -> np.ndarray:
        """proofs: the containers back to back (bytes or u8 array), commitments: ms[i] encoded points per proof back to
        back; ms: m_i per proof, or None to frame the stream first (proofs_scan; BppError when it cannot be framed)
        -> status (count,) u32: 0 Ok / 1 VerificationError / 2 FormatError"""
        raw, cm, m, count = self._block("verify_serialized_mixed", proofs, commitments, ms, uncompressed)
        ok = np.zeros(count, dtype=np.uint32)
        check(_lib.lib().bpp_range_verify_batch_serialized_mixed(
            self.handle, _some(raw), _some(cm), _some(m), count, _flags(transcript, uncompressed), _some(ok)),
            "bpp_range_verify_batch_serialized_mixed")
        return ok

    # ---- the grouped check over mixed batches (include/bpp_amd.h; the partition: mixed_groups) ----
    def grouped_mixed_workspace_bytes(self, ms, group: int = 32) -> int:
        """bytes of device workspace run_grouped_mixed_device needs (0: an m_i or the group is not taken)"""
        m = self._ms(ms)
        return _lib.lib().bpp_verifier_grouped_mixed_workspace_bytes(self.handle, _ptr(m), len(m), group)

    def run_grouped_mixed_device(self, d_points: int, d_scalars: int, ms, weight_key, index_base: int, d_out_verdicts: int,
                                 d_workspace: int, workspace_bytes: int, group: int = 32, stream: int = 0,
                                 d_challenges: int = 0, d_weights: int = 0):
        """run_mixed_device's verdict vector through the grouped check: one weighted check per group of `group` neighbours of
        the batch gathered by aggregation size (mixed_groups(ms, group) is the partition), an exact pass over the proofs of
        the groups that fail.  Input as for run_mixed_device; weight_key / d_weights (caller order) as for
        run_grouped_device.  Synchronises the stream.  -> (groups that failed, proofs re-verified exactly)"""
        m = self._ms(ms)
        stats = (ctypes.c_uint64 * 2)()
        check(_lib.lib().bpp_verifier_run_grouped_mixed(self.handle, d_points, d_scalars, _ptr(m), len(m), d_challenges or None,
                                                        _weight_key_arg(weight_key, d_weights), ctypes.c_uint64(index_base),
                                                        d_weights or None, group, d_out_verdicts, stats, d_workspace,
                                                        workspace_bytes, stream or None),
              "bpp_verifier_run_grouped_mixed")
        return int(stats[0]), int(stats[1])

    def serialized_grouped_mixed_workspace_bytes(self, ms, group: int = 32) -> int:
        """bytes of device workspace verify_serialized_grouped_mixed_device needs (0: an m_i or the group is not taken)"""
        m = self._ms(ms)
        return _lib.lib().bpp_verifier_serialized_grouped_mixed_workspace_bytes(self.handle, _ptr(m), len(m), group)

    def verify_serialized_grouped_mixed_device(self, d_proofs: int, d_commitments: int, ms, d_ok: int, d_workspace: int,
                                               workspace_bytes: int, weight_key: bytes = None, index_base: int = 0,
                                               group: int = 32, stream: int = 0, transcript: bool = False,
                                               uncompressed: bool = False):
        """verify_serialized_mixed_device's status vector with the grouped check behind the decoder.  weight_key: 32 secret
        bytes, None = os.urandom(32).  Synchronises the stream.  -> (groups that failed, proofs re-verified exactly)"""
        m = self._ms(ms)
        stats = (ctypes.c_uint64 * 2)()
        check(_lib.lib().bpp_range_verify_batch_serialized_grouped_mixed_device(
            self.handle, d_proofs, d_commitments, _ptr(m), len(m), _flags(transcript, uncompressed),
            _weight_key_arg(weight_key, 0), ctypes.c_uint64(index_base), group, d_ok, stats, d_workspace, workspace_bytes,
            stream or None), "bpp_range_verify_batch_serialized_grouped_mixed_device")
        return int(stats[0]), int(stats[1])

    def sum_partials_device(self, d_partials: int, n: int, d_ok: int, stream: int = 0):
        check(_lib.lib().bpp_verifier_sum_partials(self.handle, d_partials, n, d_ok, stream or None),
              "bpp_verifier_sum_partials")

    def prove_batch(self, values, gammas, transcript: bool = False, blind_key: bytes = None, index_base: int = 0,
                    amount64: bool = False):
        """RangeProof::prove + RangeProver::commit for `count` provers sharing this engine's (pk, n, m).
        transcript=True: challenges from the Fiat-Shamir transcript (csrc/transcript.hpp) instead of the reference's
        constants -- not a reference code path, parity unpinned.  blind_key (32 secret bytes, transcript mode only): the
        blinding values come from this key (include/bpp_amd.h "Blinding"); None = the reference's literals, which hide nothing.
        values: (count, m) ints < 2^64 ; gammas: (count, m) scalars (ints or (count, m, 4) uint64).
        Returns (points (count, 3+2k, PW), scalars (count, 3, 4), V (count, m, PW)) in wire format --
        bit-identical to RangeProof.prove / RangeProver.commit one by one.
        amount64=True (BPP_PROVE_AMOUNT64): the commitments are v g + gamma h with the whole 64-bit v instead of the
        `v as i32` of range/prover.rs:37; routed through the mixed call with every m_i = m."""
        vals = np.ascontiguousarray(np.asarray(values, dtype=np.uint64).reshape(-1, self.m))
        count = vals.shape[0]
        if amount64:
            if isinstance(gammas, np.ndarray) and gammas.dtype == np.uint64 and gammas.ndim == 3:
                grows = [[gammas[i, j] for j in range(self.m)] for i in range(count)]
            else:
                grows = [list(row) for row in gammas]
            recs, sc = self.prove_batch_mixed([[int(x) for x in row] for row in vals], grows, transcript=transcript,
                                              blind_key=blind_key, index_base=index_base, amount64=True)
            PW, nrec = self.arith.PW, 3 + 2 * self.k
            pts = np.zeros((count, nrec, PW), dtype=np.uint64)
            V = np.zeros((count, self.m, PW), dtype=np.uint64)
            for i, r in enumerate(recs):
                pts[i], V[i] = r[:nrec], r[nrec:]
            return pts, sc, V
        if isinstance(gammas, np.ndarray) and gammas.dtype == np.uint64 and gammas.ndim == 3:
            gm = np.ascontiguousarray(gammas)
        else:
            gm = np.zeros((count, self.m, 4), dtype=np.uint64)
            for i, row in enumerate(gammas):
                for j, g in enumerate(row):
                    gm[i, j] = scalar_to_wire(g)
        PW = self.arith.PW
        pts = np.zeros((count, 3 + 2 * self.k, PW), dtype=np.uint64)
        sc = np.zeros((count, 3, 4), dtype=np.uint64)
        V = np.zeros((count, self.m, PW), dtype=np.uint64)
        _prover_key(blind_key, transcript)
        if transcript:
            check(_lib.lib().bpp_range_prove_batch_fs(self.handle, _ptr(vals), _ptr(gm), count, blind_key, index_base,
                                                      _ptr(pts), _ptr(sc), _ptr(V)), "bpp_range_prove_batch_fs")
        else:
            check(_lib.lib().bpp_range_prove_batch(self.handle, _ptr(vals), _ptr(gm), count, _ptr(pts), _ptr(sc), _ptr(V)),
                  "bpp_range_prove_batch")
        return pts, sc, V

    def prover_workspace_bytes(self, count: int) -> int:
        return _lib.lib().bpp_prover_workspace_bytes(self.handle, count)

    def prove_batch_device(self, d_values: int, d_gammas: int, count: int, d_out_points: int, d_out_scalars: int,
                           d_out_V: int, d_workspace: int, workspace_bytes: int, stream: int = 0,
                           transcript: bool = False, d_out_challenges: int = 0, blind_key: bytes = None,
                           index_base: int = 0, d_blinding: int = 0):
        """prove_batch with every buffer in HBM (raw device pointers), asynchronous on `stream`.  Transcript mode: blinding
        from blind_key (32 bytes) / d_blinding (count x (5 + 2k) scalars on the device), else the reference's literals."""
        if transcript:
            check(_lib.lib().bpp_range_prove_batch_fs_device(self.handle, d_values, d_gammas, count, blind_key, index_base,
                                                             d_blinding or None, d_out_points,
                                                             d_out_scalars, d_out_V or None, d_out_challenges or None,
                                                             d_workspace, workspace_bytes, stream or None),
                  "bpp_range_prove_batch_fs_device")
            return
        check(_lib.lib().bpp_range_prove_batch_device(self.handle, d_values, d_gammas, count, d_out_points, d_out_scalars,
                                                      d_out_V or None, d_workspace, workspace_bytes, stream or None),
              "bpp_range_prove_batch_device")

    # ---- the WIP seam: WeightedInnerProductProof::{prove, verify} for any statement over this engine's key ----
    def wip_prover_workspace_bytes(self, count: int) -> int:
        return _lib.lib().bpp_wip_prover_workspace_bytes(self.handle, count)

    def wip_verifier_workspace_bytes(self, count: int, nv: int) -> int:
        return _lib.lib().bpp_wip_verifier_workspace_bytes(self.handle, count, nv)

    def wip_points_per_proof(self, nv: int) -> int:
        """wire points of a seam record [A', wip.A, wip.B, L.., R.., V_0..V_{nv-1}]"""
        return 3 + 2 * self.k + nv

    def wip_prove_device(self, d_a: int, d_b: int, d_y: int, d_gamma: int, count: int, nv: int, d_out_points: int,
                         d_out_scalars: int, d_workspace: int, workspace_bytes: int, stream: int = 0, transcript: bool = False,
                         d_transcript: int = 0, blind_key: bytes = None, index_base: int = 0, d_blinding: int = 0,
                         d_out_challenges: int = 0):
        """bpp_wip_prove_batch_device (include/bpp_amd.h): every buffer in HBM (raw device pointers), asynchronous on
        `stream`.  Writes points 1 .. 2+2k of each record of 3 + 2k + nv wire points."""
        check(_lib.lib().bpp_wip_prove_batch_device(self.handle, d_a, d_b, d_y, d_gamma, count, nv, 1 if transcript else 0,
                                                    d_transcript or None, blind_key, index_base, d_blinding or None,
                                                    d_out_points, d_out_scalars, d_out_challenges or None, d_workspace,
                                                    workspace_bytes, stream or None), "bpp_wip_prove_batch_device")

    def wip_verify_device(self, d_points: int, d_scalars: int, d_y: int, d_statement: int, nv: int, count: int, d_ok: int,
                          d_workspace: int, workspace_bytes: int, stream: int = 0, transcript: bool = False,
                          d_transcript: int = 0, d_challenges: int = 0, d_out_scalars: int = 0, d_out_result: int = 0):
        """bpp_wip_verify_batch_device (include/bpp_amd.h): every buffer in HBM, asynchronous on `stream`"""
        check(_lib.lib().bpp_wip_verify_batch_device(self.handle, d_points, d_scalars, d_y, d_statement, nv, count,
                                                     1 if transcript else 0, d_transcript or None, d_challenges or None, d_ok,
                                                     d_workspace, workspace_bytes, d_out_scalars or None,
                                                     d_out_result or None, stream or None), "bpp_wip_verify_batch_device")

    @staticmethod
    def _wip_rows(rows, width: int) -> np.ndarray:
        if isinstance(rows, np.ndarray) and rows.dtype == np.uint64:
            return np.ascontiguousarray(rows).reshape(-1, width, 4)
        out = np.zeros((len(rows), width, 4), dtype=np.uint64)
        for i, row in enumerate(rows):
            if len(row) != width:
                raise ValueError("expected %d scalars per proof" % width)
            out[i] = scalars_to_wire(list(row))
        return out

    def wip_prove_batch(self, a, b, y, gamma, nv: int = 0, points=None, transcript=None, blind_key: bytes = None,
                        index_base: int = 0, blinding=None):
        """WeightedInnerProductProof::prove for `count` statements over this engine's key (host arrays, synchronous).
        a, b: (count, len) scalars; y, gamma: (count,) scalars.  points: None, or the (count, 3+2k+nv, PW) records to
        write into (point 0 and the last nv are the caller's and come back untouched).  transcript: None (the reference's
        literal challenges) or (count, 32) uint8 running transcript states.  blinding: None or (count, 5+2k) scalars.
        -> (points, scalars (count, 3, 4), challenges (count, 1+k, 4) [e, e_1..e_k])"""
        mn = self.n * self.m
        av, bv = self._wip_rows(a, mn), self._wip_rows(b, mn)
        count = av.shape[0]
        yv, gv = scalars_to_wire(y).reshape(count, 4), scalars_to_wire(gamma).reshape(count, 4)
        PW = self.arith.PW
        npts = self.wip_points_per_proof(nv)
        pts = (np.zeros((count, npts, PW), dtype=np.uint64) if points is None
               else np.ascontiguousarray(points, dtype=np.uint64).reshape(count, npts, PW).copy())
        tr = None if transcript is None else np.ascontiguousarray(transcript, dtype=np.uint8).reshape(count, 32)
        bl = None if blinding is None else self._wip_rows(blinding, 5 + 2 * self.k)
        sc = np.zeros((count, 3, 4), dtype=np.uint64)
        ch = np.zeros((count, 1 + self.k, 4), dtype=np.uint64)
        check(_lib.lib().bpp_wip_prove_batch(self.handle, _ptr(av), _ptr(bv), _ptr(yv), _ptr(gv), count, nv,
                                             0 if tr is None else 1, _ptr(tr), blind_key, index_base, _ptr(bl), _ptr(pts),
                                             _ptr(sc), _ptr(ch)), "bpp_wip_prove_batch")
        return pts, sc, ch

    def wip_verify_batch(self, points, scalars, y, statement, nv: int, transcript=None, challenges=None,
                         want_scalars: bool = False, want_result: bool = False):
        """WeightedInnerProductProof::verify for `count` proofs (host arrays, synchronous).  points: (count, 3+2k+nv, PW)
        records [A', wip.A, wip.B, L.., R.., V..]; scalars: (count, 3, 4); y: (count,); statement: (count, 2 len + 1 + nv)
        scalars [Gc, Hc, gc, Vc].  challenges: None or (count, 1+k) scalars [e, e_1..e_k].  -> ok (count,) u32, and with
        want_scalars / want_result also the MulVec scalars (count, N, 4) / the sums (count, PW)"""
        mn = self.n * self.m
        PW = self.arith.PW
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, self.wip_points_per_proof(nv), PW)
        count = pts.shape[0]
        sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(count, 3, 4)
        yv = scalars_to_wire(y).reshape(count, 4)
        stm = self._wip_rows(statement, 2 * mn + 1 + nv)
        if stm.shape[0] != count:
            raise RuntimeError("wip_verify_batch: one statement per proof record")
        tr = None if transcript is None else np.ascontiguousarray(transcript, dtype=np.uint8).reshape(count, 32)
        ch = None if challenges is None else self._wip_rows(challenges, 1 + self.k)
        ok = np.zeros(count, dtype=np.uint32)
        osc = np.zeros((count, 2 * mn + 2 * self.k + 5 + nv, 4), dtype=np.uint64) if want_scalars else None
        ores = np.zeros((count, PW), dtype=np.uint64) if want_result else None
        check(_lib.lib().bpp_wip_verify_batch(self.handle, _ptr(pts), _ptr(sc), _ptr(yv), _ptr(stm), nv, count,
                                              0 if tr is None else 1, _ptr(tr), _ptr(ch), _ptr(ok), _ptr(osc), _ptr(ores)),
              "bpp_wip_verify_batch")
        if want_scalars or want_result:
            return ok, osc, ores
        return ok

    # ---- commitments for a block of amounts through the engine's tables (include/bpp_amd.h) ----
    def commit_batch_device(self, d_values: int, d_gammas: int, count: int, d_out_V: int, stream: int = 0,
                            amount64: bool = False):
        """RangeProver::commit (range/prover.rs:28-42) for `count` resident values and gammas over this engine's g and h:
        d_out_V receives count wire points.  amount64=False keeps the `v as i32` of prover.rs:37.  Only enqueues."""
        check(_lib.lib().bpp_commit_batch_device(self.handle, d_values, d_gammas, count, _flags(amount64=amount64), d_out_V,
                                                 stream or None), "bpp_commit_batch_device")

    def commit_batch(self, values, gammas, amount64: bool = False) -> np.ndarray:
        """values: count ints < 2^64; gammas: count scalars (ints or (count, 4) uint64) -> (count, PW) wire points,
        s g + gamma h with s = new(v as i32) (range/prover.rs:37; equal to RangeProver.commit one by one) or, amount64=True,
        the whole value"""
        vals = np.ascontiguousarray(np.asarray([int(x) for x in values], dtype=np.uint64))
        count = len(vals)
        if isinstance(gammas, np.ndarray) and gammas.dtype == np.uint64 and gammas.ndim == 2:
            gm = np.ascontiguousarray(gammas)
        else:
            gm = scalars_to_wire(gammas) if count else np.zeros((0, 4), dtype=np.uint64)
        if len(gm) != count:
            raise RuntimeError("one gamma per value")
        out = np.zeros((count, self.arith.PW), dtype=np.uint64)
        check(_lib.lib().bpp_commit_batch(self.handle, _some(vals), _some(gm), count, _flags(amount64=amount64), _some(out)),
              "bpp_commit_batch")
        return out

    # ---- proving blocks of mixed aggregation sizes: proof i has ms[i] values (include/bpp_amd.h) ----
    def prover_mixed_workspace_bytes(self, ms, serialized: bool = False) -> int:
        """bytes of device workspace prove_mixed_device (serialized: prove_serialized_mixed_device) needs (0: an m_i is
        not taken)"""
        m = self._ms(ms)
        f = _lib.lib().bpp_prover_serialized_mixed_workspace_bytes if serialized else _lib.lib().bpp_prover_mixed_workspace_bytes
        return f(self.handle, _some(m), len(m))

    def prove_mixed_device(self, d_values: int, d_gammas: int, ms, d_out_points: int, d_out_scalars: int, d_workspace: int,
                           workspace_bytes: int, stream: int = 0, transcript: bool = False, d_out_challenges: int = 0,
                           blind_key: bytes = None, index_base: int = 0, d_blinding: int = 0, amount64: bool = False):
        """RangeProof::prove for a resident block in which proof i has ms[i] values (packed in caller order, as the gammas),
        each against the prefix key PublicKey::new(n ms[i]).  d_out_points receives the packed records [A, wip.A, wip.B,
        L.., R.., V..] run_mixed_device reads, d_out_scalars (count, 3) scalars, d_out_challenges the packed challenge
        blocks.  Proof i's blinding index is index_base + i.  Blocks while it uploads the per-proof index.
        amount64=True (BPP_PROVE_AMOUNT64): commitments over the whole 64-bit values, not `v as i32` (range/prover.rs:37)."""
        m = self._ms(ms)
        check(_lib.lib().bpp_range_prove_batch_mixed_device(
            self.handle, d_values, d_gammas, _some(m), len(m), _flags(transcript, amount64=amount64), blind_key,
            ctypes.c_uint64(index_base), d_blinding or None, d_out_points, d_out_scalars, d_out_challenges or None, d_workspace,
            workspace_bytes, stream or None), "bpp_range_prove_batch_mixed_device")

    def prove_serialized_mixed_device(self, d_values: int, d_gammas: int, ms, d_out_proofs: int, d_out_commitments: int,
                                      d_workspace: int, workspace_bytes: int, stream: int = 0, transcript: bool = False,
                                      uncompressed: bool = False, blind_key: bytes = None, index_base: int = 0,
                                      d_blinding: int = 0, amount64: bool = False):
        """prove_mixed_device with the proofs written as containers packed back to back in caller order and ms[i] encoded
        commitments per proof: the two inputs of verify_serialized_mixed_device"""
        m = self._ms(ms)
        check(_lib.lib().bpp_range_prove_batch_serialized_mixed_device(
            self.handle, d_values, d_gammas, _some(m), len(m), _flags(transcript, uncompressed, amount64), blind_key,
            ctypes.c_uint64(index_base), d_blinding or None,
            d_out_proofs, d_out_commitments, d_workspace, workspace_bytes, stream or None),
            "bpp_range_prove_batch_serialized_mixed_device")

    def _mixed_inputs(self, values, gammas):
        """values, gammas: one sequence per proof -> (packed values, packed gammas (sum m_i, 4), ms)"""
        ms = np.array([len(v) for v in values], dtype=np.uint32)
        if len(gammas) != len(values) or any(len(g) != len(v) for g, v in zip(gammas, values)):
            raise RuntimeError("one gamma per value")
        vals = np.array([int(x) for v in values for x in v], dtype=np.uint64)
        gm = np.zeros((len(vals), 4), dtype=np.uint64)
        j = 0
        for row in gammas:
            for g in row:
                gm[j] = np.asarray(g, dtype=np.uint64) if isinstance(g, np.ndarray) else scalar_to_wire(g)
                j += 1
        return vals, gm, ms

    def prove_batch_mixed(self, values, gammas, transcript: bool = False, blind_key: bytes = None, index_base: int = 0,
                          challenges: bool = False, amount64: bool = False):
        """values[i], gammas[i]: the m_i values and gammas of proof i (m_i a power of two <= m).  -> (records, scalars):
        records[i] the (mixed_points(m_i), PW) wire record [A, wip.A, wip.B, L.., R.., V..] of proof i, bit for bit what
        a dedicated (n, m_i) engine of the same key proves; scalars (count, 3, 4).  challenges=True: also the list of
        per-proof challenge blocks (3 + k_i, 4).  amount64=True (BPP_PROVE_AMOUNT64): each V is v g + gamma h over the whole
        64-bit value instead of the `v as i32` of range/prover.rs:37, so amounts of 2^31 and more prove and verify."""
        _prover_key(blind_key, transcript)
        vals, gm, ms = self._mixed_inputs(values, gammas)
        count, PW = len(ms), self.arith.PW
        taken = self._taken(ms)
        npts = [self.mixed_points(int(x)) if taken else 0 for x in ms]
        nch = [3 + self._rounds(int(x)) if taken else 0 for x in ms]
        pts = np.zeros((max(sum(npts), 1), PW), dtype=np.uint64)
        sc = np.zeros((count, 3, 4), dtype=np.uint64)
        ch = np.zeros((max(sum(nch), 1), 4), dtype=np.uint64)
        check(_lib.lib().bpp_range_prove_batch_mixed(
            self.handle, _some(vals), _some(gm), _some(ms), count, _flags(transcript, amount64=amount64), blind_key,
            ctypes.c_uint64(index_base), _ptr(pts), _some(sc), _ptr(ch) if challenges else None),
            "bpp_range_prove_batch_mixed")
        po, co = np.concatenate([[0], np.cumsum(npts)]).astype(int), np.concatenate([[0], np.cumsum(nch)]).astype(int)
        recs = [pts[po[i]:po[i + 1]] for i in range(count)]
        if challenges:
            return recs, sc, [ch[co[i]:co[i + 1]] for i in range(count)]
        return recs, sc

    def prove_serialized_mixed(self, values, gammas, transcript: bool = False, blind_key: bytes = None, index_base: int = 0,
                               uncompressed: bool = False, amount64: bool = False):
        """prove_batch_mixed as bytes -> (proofs, commitments, ms): the containers back to back in caller order, ms[i]
        encoded commitments per proof back to back -- what verify_serialized_mixed takes, and a stream proofs_scan frames"""
        _prover_key(blind_key, transcript)
        vals, gm, ms = self._mixed_inputs(values, gammas)
        count, version = len(ms), 2 if uncompressed else 1
        pb = uncompressed_bytes(self.arith) if uncompressed else compressed_bytes(self.arith)
        nbytes = sum(proof_bytes(self.arith, self.n, int(x), version) for x in ms) if self._taken(ms) and pb else 0
        raw = np.zeros(max(nbytes, 1), dtype=np.uint8)
        cm = np.zeros(max(int(ms.sum()) * pb, 1), dtype=np.uint8)
        check(_lib.lib().bpp_range_prove_batch_serialized_mixed(
            self.handle, _some(vals), _some(gm), _some(ms), count, _flags(transcript, uncompressed, amount64), blind_key,
            ctypes.c_uint64(index_base), _ptr(raw), _ptr(cm)), "bpp_range_prove_batch_serialized_mixed")
        return raw[:nbytes].tobytes(), cm[:int(ms.sum()) * pb].tobytes(), ms

    # ---- mask recovery and scanning: the receiver's side (include/bpp_amd.h "mask recovery") ----
    def _blinding_args(self, blind_key, index, blinding, count: int, ms):
        """host-side blinding arguments of the recovery calls -> (key, index array or None, blinding array or None)"""
        if blind_key is not None and len(blind_key) != 32:
            raise ValueError("blind_key: 32 bytes")
        idx, bl = _index_arg(index, count, "one index per proof"), None
        if blinding is not None:
            if isinstance(blinding, np.ndarray) and blinding.dtype == np.uint64:
                bl = np.ascontiguousarray(blinding).reshape(-1, 4)
            else:
                bl = scalars_to_wire([int(x) for row in blinding for x in row])
            if self._taken(ms):
                need = sum(5 + 2 * self._rounds(int(x)) for x in ms)
                if len(bl) != need:
                    raise RuntimeError("blinding: 5 + 2 k_i scalars per proof (%d in all), got %d" % (need, len(bl)))
        return blind_key, idx, bl

    def recover_workspace_bytes(self, ms, serialized: bool = False) -> int:
        """bytes of device workspace recover_masks_device (serialized: scan_serialized_mixed_device) needs (0: an m_i is
        not taken)"""
        m = self._ms(ms)
        f = _lib.lib().bpp_scan_serialized_mixed_workspace_bytes if serialized else _lib.lib().bpp_recover_mixed_workspace_bytes
        return f(self.handle, _some(m), len(m))

    def recover_masks_device(self, d_scalars: int, ms, d_out_masks: int, d_workspace: int, workspace_bytes: int,
                             stream: int = 0, d_challenges: int = 0, blind_key: bytes = None, index_base: int = 0,
                             d_index: int = 0, d_blinding: int = 0):
        """Gamma_i = gamma_0 + z^2 gamma_1 + .. of every proof of a resident mixed batch, from its scalar triple, its
        challenge block (d_challenges: the packed blocks derive_challenges_mixed_device writes; 0: the literals) and its
        blinding: blind_key with index d_index[i] or index_base + i, or d_blinding, or the literals.  For ms[i] = 1
        Gamma_i is the output's mask.  Not a verification.  d_out_masks: (count, 4) u64 in caller order."""
        m = self._ms(ms)
        check(_lib.lib().bpp_range_recover_masks_mixed_device(
            self.handle, d_scalars, _some(m), len(m), d_challenges or None, blind_key,
            ctypes.c_uint64(index_base), d_index or None, d_blinding or None, d_out_masks, d_workspace, workspace_bytes,
            stream or None), "bpp_range_recover_masks_mixed_device")

    def recover_masks(self, scalars, ms, challenges=None, blind_key: bytes = None, index_base: int = 0, index=None,
                      blinding=None) -> list:
        """scalars (count, 3, 4); ms: m_i per proof; challenges: None (the literals) or the per-proof blocks (a list of
        (3 + k_i, 4) arrays or one packed array); index: None or one blinding index per proof; blinding: None or per proof
        its 5 + 2 k_i scalars -> [Gamma_i] as ints (bpp_range_recover_masks_mixed)"""
        m = self._ms(ms)
        count = len(m)
        sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 3, 4)
        if sc.shape[0] != count:
            raise RuntimeError("recover_masks: one scalar triple per proof")
        key, idx, bl = self._blinding_args(blind_key, index, blinding, count, m)
        ch = None
        if challenges is not None:
            ch = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint64).reshape(-1, 4) for c in challenges])
                                      if isinstance(challenges, (list, tuple)) else
                                      np.asarray(challenges, dtype=np.uint64).reshape(-1, 4))
            if self._taken(m):
                need = sum(3 + self._rounds(int(x)) for x in m)
                if len(ch) != need:
                    raise RuntimeError("recover_masks: 3 + k_i challenges per proof (%d in all), got %d" % (need, len(ch)))
        out = np.zeros((count, 4), dtype=np.uint64)
        check(_lib.lib().bpp_range_recover_masks_mixed(
            self.handle, _some(sc), _some(m), count, _ptr(ch), key, ctypes.c_uint64(index_base), _ptr(idx), _ptr(bl),
            _some(out)), "bpp_range_recover_masks_mixed")
        return [wire_to_int(x) for x in out]

    def scan_serialized_mixed_device(self, d_proofs: int, d_commitments: int, ms, d_out_masks: int, d_status: int,
                                     d_workspace: int, workspace_bytes: int, stream: int = 0, transcript: bool = False,
                                     uncompressed: bool = False, amount64: bool = False, blind_key: bytes = None,
                                     index_base: int = 0, d_index: int = 0, d_blinding: int = 0, d_amounts: int = 0):
        """Scans a resident block of containers (verify_serialized_mixed_device's input) for the outputs of a key: decoder,
        challenges, Gamma_i, and for ms[i] = 1 with a candidate amount d_amounts[i] the test V_0 == v g + Gamma h.
        d_status[i]: 0 the output is the key's and d_out_masks[i] its mask / 1 it is not (mask zero) / 2 FormatError (mask
        zero) / 3 unconfirmed -- no amount, or ms[i] > 1 (Gamma as computed).  A scan is not a verification."""
        m = self._ms(ms)
        check(_lib.lib().bpp_range_scan_serialized_mixed_device(
            self.handle, d_proofs, d_commitments, _some(m), len(m), _flags(transcript, uncompressed, amount64), blind_key,
            ctypes.c_uint64(index_base), d_index or None, d_blinding or None, d_amounts or None, d_out_masks, d_status,
            d_workspace, workspace_bytes, stream or None), "bpp_range_scan_serialized_mixed_device")

    def scan_serialized_mixed(self, proofs, commitments, ms=None, transcript: bool = False, uncompressed: bool = False,
                              amount64: bool = False, blind_key: bytes = None, index_base: int = 0, index=None,
                              blinding=None, amounts=None):
        """proofs, commitments, ms: as verify_serialized_mixed; amounts: None or one candidate amount per proof (read for
        ms[i] = 1) -> (status (count,) u32, [Gamma_i] as ints); see scan_serialized_mixed_device for the status words"""
        raw, cm, m, count = self._block("scan_serialized_mixed", proofs, commitments, ms, uncompressed)
        key, idx, bl = self._blinding_args(blind_key, index, blinding, count, m)
        am = None if amounts is None else \
            _amounts_arg(amounts, count, "scan_serialized_mixed: one candidate amount per proof")
        masks = np.zeros((count, 4), dtype=np.uint64)
        status = np.zeros(count, dtype=np.uint32)
        check(_lib.lib().bpp_range_scan_serialized_mixed(
            self.handle, _some(raw), _some(cm), _some(m), count, _flags(transcript, uncompressed, amount64), key,
            ctypes.c_uint64(index_base), _ptr(idx), _ptr(bl), _ptr(am), _some(masks), _some(status)),
            "bpp_range_scan_serialized_mixed")
        return status, [wire_to_int(x) for x in masks]

    def scan_keys_workspace_bytes(self, ms, n_keys: int) -> int:
        """bytes of device workspace scan_serialized_mixed_keys_device needs (0: an m_i is not taken, or n_keys x count is
        over the bound)"""
        m = self._ms(ms)
        return _lib.lib().bpp_scan_serialized_mixed_keys_workspace_bytes(self.handle, _some(m), len(m), n_keys)

    def scan_serialized_mixed_keys_device(self, d_proofs: int, d_commitments: int, ms, d_keys: int, n_keys: int,
                                          d_out_masks: int, d_status: int, d_workspace: int, workspace_bytes: int,
                                          stream: int = 0, transcript: bool = True, uncompressed: bool = False,
                                          amount64: bool = False, index_base: int = 0, d_index: int = 0, d_amounts: int = 0):
        """scan_serialized_mixed_device for n_keys view keys in one call: decoder, membership test, challenges and the
        inversions once, the key-dependent part per (key, proof) pair.  d_keys: n_keys x 32 bytes; the blinding index of
        proof i (d_index[i] or index_base + i) is shared by all keys; d_amounts (n_keys, count) u64, d_out_masks
        (n_keys, count, 4) u64 and d_status (n_keys, count) u32 are key-major.  The status words are the single-key call's.
        Every key is a view key; a scan is not a verification."""
        m = self._ms(ms)
        check(_lib.lib().bpp_range_scan_serialized_mixed_keys_device(
            self.handle, d_proofs, d_commitments, _some(m), len(m), _flags(transcript, uncompressed, amount64), d_keys or None,
            n_keys, ctypes.c_uint64(index_base), d_index or None, d_amounts or None, d_out_masks, d_status, d_workspace,
            workspace_bytes, stream or None), "bpp_range_scan_serialized_mixed_keys_device")

    def scan_serialized_mixed_keys(self, proofs, commitments, ms=None, keys=(), transcript: bool = True,
                                   uncompressed: bool = False, amount64: bool = False, index_base: int = 0, index=None,
                                   amounts=None):
        """proofs, commitments, ms: as scan_serialized_mixed; keys: a list of 32-byte strings; index: None or one blinding
        index per proof, shared by all keys; amounts: None or K x count candidate amounts (amounts[j][i]: proof i under key
        j) -> (status (K, count) u32, masks: K lists of count ints) (bpp_range_scan_serialized_mixed_keys)"""
        where = "scan_serialized_mixed_keys"
        with _packed_keys(where, keys) as (kb, nk):
            raw, cm, m, count = self._block(where, proofs, commitments, ms, uncompressed)
            idx = _index_arg(index, count, where + ": one blinding index per proof")
            am = None if amounts is None else \
                _amounts_arg(amounts, nk * count, where + ": K x count candidate amounts", rows=True)
            masks = np.zeros((nk, count, 4), dtype=np.uint64)
            status = np.zeros((nk, count), dtype=np.uint32)
            some = nk > 0 and count > 0
            check(_lib.lib().bpp_range_scan_serialized_mixed_keys(
                self.handle, _some(raw), _some(cm), _some(m), count, _flags(transcript, uncompressed, amount64), _ptr(kb), nk,
                ctypes.c_uint64(index_base), _ptr(idx), _ptr(am) if some else None, _ptr(masks) if some else None,
                _ptr(status) if some else None), "bpp_range_scan_serialized_mixed_keys")
        return status, [[wire_to_int(x) for x in row] for row in masks]

    # ---- sealed amounts; verifying a block and listing the outputs of many keys (include/bpp_amd.h) ----
    def seal_amounts_device(self, blind_key: bytes, d_in: int, count: int, d_out: int, stream: int = 0, index_base: int = 0,
                            d_index: int = 0):
        """d_out[i] = d_in[i] XOR pad(blind_key, d_index[i] or index_base + i) over count resident u64: seals amounts, and
        opens sealed ones (bpp_amounts_seal_device).  d_in and d_out may be the same buffer."""
        check(_lib.lib().bpp_amounts_seal_device(self.arith.handle, blind_key, ctypes.c_uint64(index_base), d_index or None,
                                                 d_in or None, count, d_out or None, stream or None), "bpp_amounts_seal_device")

    def seal_amounts(self, blind_key: bytes, amounts, index_base: int = 0, index=None) -> np.ndarray:
        """amounts: ints below 2^64; index: None or one blinding index per amount -> (count,) u64, amount XOR pad; applied
        to sealed amounts it opens them (bpp_amounts_seal)"""
        am = _amounts_arg(amounts)
        idx = _index_arg(index, len(am), "seal_amounts: one blinding index per amount")
        out = np.zeros(len(am), dtype=np.uint64)
        check(_lib.lib().bpp_amounts_seal(self.arith.handle, blind_key, ctypes.c_uint64(index_base), _ptr(idx), _some(am),
                                          len(am), _some(out)), "bpp_amounts_seal")
        return out

    def view_tags_device(self, blind_key: bytes, count: int, d_out: int, stream: int = 0, index_base: int = 0, d_index: int = 0):
        """d_out[i] = view_tag(blind_key, d_index[i] or index_base + i) over count resident bytes: the byte a sender
        attaches to an output next to its sealed amount (bpp_view_tags_device)"""
        check(_lib.lib().bpp_view_tags_device(self.arith.handle, blind_key, ctypes.c_uint64(index_base), d_index or None, count,
                                              d_out or None, stream or None), "bpp_view_tags_device")

    def view_tags(self, blind_key: bytes, count: int = None, index_base: int = 0, index=None) -> np.ndarray:
        """count outputs from index_base, or one blinding index per output -> (count,) u8, the first byte of
        SHA-256(key || "bppt" || index || 0 || 0) (bpp_view_tags).  The tag authenticates nothing."""
        idx = _index_arg(index, count, "view_tags: one blinding index per output")
        count = int(count or 0) if idx is None else len(idx)
        out = np.zeros(count, dtype=np.uint8)
        check(_lib.lib().bpp_view_tags(self.arith.handle, blind_key, ctypes.c_uint64(index_base), _some(idx), count, _some(out)),
              "bpp_view_tags")
        return out

    def verify_find_tagged_workspace_bytes(self, ms, n_keys: int) -> int:
        """bytes of device workspace verify_find_serialized_mixed_keys_device needs when d_tags is given (0 where
        verify_find_workspace_bytes gives 0): room for every pair being a candidate"""
        m = self._ms(ms)
        return _lib.lib().bpp_verify_find_tagged_workspace_bytes(self.handle, _some(m), len(m), n_keys)

    def verify_find_workspace_bytes(self, ms, n_keys: int) -> int:
        """bytes of device workspace verify_find_serialized_mixed_keys_device needs (0: an m_i is not taken, or
        n_keys x count is over the bound); grows with n_keys"""
        m = self._ms(ms)
        return _lib.lib().bpp_verify_find_serialized_mixed_keys_workspace_bytes(self.handle, _some(m), len(m),
                                                                                n_keys)

    def verify_find_serialized_mixed_keys_device(self, d_proofs: int, d_commitments: int, ms, d_keys: int, n_keys: int,
                                                 d_amounts: int, d_ok: int, d_hits: int, max_hits: int, d_n_hits: int,
                                                 d_workspace: int, workspace_bytes: int, stream: int = 0,
                                                 uncompressed: bool = False, amount64: bool = False, sealed: bool = False,
                                                 index_base: int = 0, d_index: int = 0, d_tags: int = 0, d_n_candidates: int = 0):
        """Verifies a resident block (d_ok: verify_serialized_mixed_device's words under the transcript) and lists the
        single outputs that belong to the n_keys view keys at d_keys, the front run once.  d_amounts: sealed -- count u64
        sealed amounts shared by all keys; else (n_keys, count) u64 candidates, key-major.  d_hits: max_hits records of 12
        u32 [key number, position, amount lo, hi, mask as 8 words] in ascending (key number, position); d_n_hits: one u32,
        the hits found -- above max_hits, only the first max_hits are written.  A hit is a VERIFIED single output whose
        commitment opens to the amount and the mask recovered under that key.  d_tags (None or 0: the untagged entry):
        count resident view-tag bytes, shared by all keys -- the tagged entry, which rules a pair out after one hash when
        its tag does not match, takes verify_find_tagged_workspace_bytes of workspace and writes the number of pairs that
        passed the tag test to d_n_candidates (one u32) when that is given."""
        m = self._ms(ms)
        head = (self.handle, d_proofs, d_commitments, _some(m), len(m), _flags(True, uncompressed, amount64, sealed),
                d_keys or None, n_keys, ctypes.c_uint64(index_base), d_index or None, d_amounts or None, d_ok or None,
                d_hits or None, max_hits, d_n_hits or None)
        tail = (d_workspace, workspace_bytes, stream or None)
        if d_tags:
            check(_lib.lib().bpp_range_verify_find_tagged_serialized_mixed_keys_device(*head, d_tags, d_n_candidates or None,
                                                                                       *tail),
                  "bpp_range_verify_find_tagged_serialized_mixed_keys_device")
        else:
            check(_lib.lib().bpp_range_verify_find_serialized_mixed_keys_device(*head, *tail),
                  "bpp_range_verify_find_serialized_mixed_keys_device")

    def verify_find_serialized_mixed_keys(self, proofs, commitments, ms=None, keys=(), amounts=(), sealed: bool = False,
                                          uncompressed: bool = False, amount64: bool = False, index_base: int = 0, index=None,
                                          max_hits: int = None, tags=None):
        """proofs, commitments, ms, keys, index: as scan_serialized_mixed_keys; amounts: sealed -- one sealed amount per
        proof; else K x count candidates (amounts[j][i]: proof i under key j); max_hits: None for room for every pair
        -> (ok (count,) u32, hits, found): ok as verify_serialized_mixed under the transcript; hits the list of
        (key_no, position, amount, mask) in ascending (key_no, position), at most max_hits of them; found the number of
        hits there are (bpp_range_verify_find_serialized_mixed_keys).  With no keys the block is verified all the same
        and no hit is listed.  tags (None or 0: the untagged entry): one view-tag byte per proof, shared by all keys -- a pair
        whose tag does not match its key is ruled out after one hash, and the result is (ok, hits, found, candidates) with
        candidates the number of pairs that passed the tag test (bpp_range_verify_find_tagged_serialized_mixed_keys)."""
        where = "verify_find_serialized_mixed_keys"
        with _packed_keys(where, keys) as (kb, nk):
            raw, cm, m, count = self._block(where, proofs, commitments, ms, uncompressed)
            idx = _index_arg(index, count, where + ": one blinding index per proof")
            if sealed:
                am = _amounts_arg(amounts, count, where + ": one sealed amount per proof")
            else:
                am = _amounts_arg(amounts, nk * count, where + ": K x count candidate amounts", rows=True)
            tg = None
            if tags is not None and not (isinstance(tags, int) and tags == 0):
                tg = _tags_arg(tags)
                if len(tg) != count:
                    raise RuntimeError(where + ": one view tag per proof")
            cap = nk * count if max_hits is None else int(max_hits)
            ok = np.zeros(count, dtype=np.uint32)
            rec = np.zeros((cap, 12), dtype=np.uint32)
            found = np.zeros(1, dtype=np.uint32)
            cands = np.zeros(1, dtype=np.uint32)
            some = nk > 0 and count > 0
            head = (self.handle, _some(raw), _some(cm), _some(m), count, _flags(True, uncompressed, amount64, sealed), _ptr(kb),
                    nk, ctypes.c_uint64(index_base), _ptr(idx), _ptr(am) if some else None, _some(ok), _some(rec), cap,
                    _ptr(found))
            if tg is None:
                check(_lib.lib().bpp_range_verify_find_serialized_mixed_keys(*head),
                      "bpp_range_verify_find_serialized_mixed_keys")
            else:
                check(_lib.lib().bpp_range_verify_find_tagged_serialized_mixed_keys(*head, _ptr(tg) if some else None,
                                                                                    _ptr(cands)),
                      "bpp_range_verify_find_tagged_serialized_mixed_keys")
        n = int(found[0])
        return (ok, _hits(rec, n), n) if tg is None else (ok, _hits(rec, n), n, int(cands[0]))

    # ---- outputs with masks derived from their recipients' keys, aggregated proofs included (include/bpp_amd.h) ----
    def make_outputs_device(self, d_keys: int, d_index: int, d_j: int, d_amounts: int, n_out: int, d_out_masks: int = 0,
                            d_out_sealed: int = 0, d_out_tags: int = 0, stream: int = 0):
        """The sender's call over n_out resident outputs (bpp_outputs_make_device): d_keys n_out x 32 bytes (the recipient's
        key of each), d_index n_out u64 (the blinding index of the output's proof), d_j n_out u32 (its place in the proof),
        d_amounts n_out u64 -> d_out_masks n_out x 4 u64 (the d_gamma layout of commit_batch_device and the mixed prove
        calls), d_out_sealed n_out u64, d_out_tags n_out bytes; each output may be 0 and is then skipped.  Only enqueues."""
        check(_lib.lib().bpp_outputs_make_device(self.arith.handle, d_keys or None, d_index or None, d_j or None, d_amounts or None,
                                                 n_out, d_out_masks or None, d_out_sealed or None, d_out_tags or None,
                                                 stream or None), "bpp_outputs_make_device")

    def make_outputs(self, keys, amounts, ms, index_base: int = 0, index=None):
        """keys: one 32-byte recipient key per OUTPUT; amounts: one int below 2^64 per output; ms: the outputs per proof, in
        order (sum(ms) outputs); index: None or one blinding index per PROOF -> (masks (n_out, 4) u64, sealed (n_out,) u64,
        tags (n_out,) u8): output j of proof i under output_mask / output_pad / output_tag(key, index of i, j)
        (bpp_outputs_make).  The masks are secret."""
        m = [int(x) for x in ms]
        with _packed_keys("make_outputs", keys) as (kb, nk):
            am = _amounts_arg(amounts)
            n_out = sum(m)
            if nk != n_out or len(am) != n_out:
                raise RuntimeError("make_outputs: one key and one amount per output, sum(ms) of them")
            pidx = _index_arg(index, len(m), "make_outputs: one blinding index per proof")
            if pidx is None:
                pidx = np.uint64(index_base) + np.arange(len(m), dtype=np.uint64)
            reps = np.asarray(m, dtype=np.int64)
            idx = np.ascontiguousarray(np.repeat(pidx, reps))
            first = np.repeat(np.cumsum(reps) - reps, reps)
            j = np.ascontiguousarray((np.arange(n_out, dtype=np.int64) - first).astype(np.uint32))
            masks = np.zeros((n_out, 4), dtype=np.uint64)
            sealed = np.zeros(n_out, dtype=np.uint64)
            tags = np.zeros(n_out, dtype=np.uint8)
            if n_out:
                check(_lib.lib().bpp_outputs_make(self.arith.handle, _ptr(kb), _ptr(idx), _ptr(j), _ptr(am), n_out, _ptr(masks),
                                                  _ptr(sealed), _ptr(tags)), "bpp_outputs_make")
        return masks, sealed, tags

    def verify_find_outputs_workspace_bytes(self, ms, n_keys: int) -> int:
        """bytes of device workspace verify_find_outputs_serialized_mixed_keys_device needs (0: an m_i is not taken, or
        n_keys x sum(ms) is over the bound)"""
        m = self._ms(ms)
        return _lib.lib().bpp_verify_find_outputs_workspace_bytes(self.handle, _some(m), len(m), n_keys)

    def verify_find_outputs_serialized_mixed_keys_device(self, d_proofs: int, d_commitments: int, ms, d_keys: int, n_keys: int,
                                                         d_sealed: int, d_tags: int, d_ok: int, d_hits: int, max_hits: int,
                                                         d_n_hits: int, d_workspace: int, workspace_bytes: int, stream: int = 0,
                                                         uncompressed: bool = False, amount64: bool = False, index_base: int = 0,
                                                         d_index: int = 0, d_n_candidates: int = 0):
        """Verifies a resident block (d_ok: verify_serialized_mixed_device's words under the transcript) and lists, per
        OUTPUT, what belongs to the n_keys view keys at d_keys, aggregated proofs included.  d_sealed: sum(ms) u64 and
        d_tags: sum(ms) bytes, per output in caller order, shared by all keys.  d_hits: max_hits records of 12 u32 [key
        number, output number, amount lo, hi, mask as 8 words] in ascending (key number, output number); d_n_hits: one u32,
        the hits found; d_n_candidates: 0 or one u32, the pairs that passed the tag test
        (bpp_range_verify_find_outputs_serialized_mixed_keys_device)."""
        m = self._ms(ms)
        check(_lib.lib().bpp_range_verify_find_outputs_serialized_mixed_keys_device(
            self.handle, d_proofs, d_commitments, _some(m), len(m), _flags(True, uncompressed, amount64), d_keys or None, n_keys,
            ctypes.c_uint64(index_base), d_index or None, d_sealed or None, d_tags or None, d_ok or None, d_hits or None, max_hits, d_n_hits or None,
            d_n_candidates or None, d_workspace, workspace_bytes, stream or None),
            "bpp_range_verify_find_outputs_serialized_mixed_keys_device")

    def verify_find_outputs_serialized_mixed_keys(self, proofs, commitments, ms=None, keys=(), sealed=(), tags=(),
                                                  uncompressed: bool = False, amount64: bool = False, index_base: int = 0,
                                                  index=None, max_hits: int = None):
        """proofs, commitments, ms, keys, index: as verify_find_serialized_mixed_keys; sealed, tags: one sealed amount and
        one tag byte per OUTPUT (sum(ms) of each), in caller order -> (ok (count,) u32, hits, found, n_candidates): ok as
        verify_serialized_mixed under the transcript; hits the list of (key_no, output_no, amount, mask) in ascending
        (key_no, output_no), at most max_hits of them (None: room for every pair); found the number of hits there are;
        n_candidates the pairs that passed the tag test (bpp_range_verify_find_outputs_serialized_mixed_keys).  With no
        keys the block is verified all the same and no hit is listed."""
        where = "verify_find_outputs_serialized_mixed_keys"
        with _packed_keys(where, keys) as (kb, nk):
            raw, cm, m, count = self._block(where, proofs, commitments, ms, uncompressed)
            n_out = int(m.sum())
            idx = _index_arg(index, count, where + ": one blinding index per proof")
            se, tg = _amounts_arg(sealed), _tags_arg(tags)
            if nk and (len(se) != n_out or len(tg) != n_out):
                raise RuntimeError(where + ": one sealed amount and one tag per output")
            cap = nk * n_out if max_hits is None else int(max_hits)
            ok = np.zeros(count, dtype=np.uint32)
            rec = np.zeros((cap, 12), dtype=np.uint32)
            found = np.zeros(1, dtype=np.uint32)
            cands = np.zeros(1, dtype=np.uint32)
            some = nk > 0 and count > 0
            check(_lib.lib().bpp_range_verify_find_outputs_serialized_mixed_keys(
                self.handle, _some(raw), _some(cm), _some(m), count, _flags(True, uncompressed, amount64), _ptr(kb), nk,
                ctypes.c_uint64(index_base), _ptr(idx), _ptr(se) if some else None, _ptr(tg) if some else None, _some(ok),
                _some(rec), cap, _ptr(found), _ptr(cands)), "bpp_range_verify_find_outputs_serialized_mixed_keys")
        n = int(found[0])
        return ok, _hits(rec, n), n, int(cands[0])

    # ---- proofs over any number of outputs (include/bpp_amd.h "proofs over ANY number of outputs") ----
    def _outs(self, outs) -> np.ndarray:
        return np.ascontiguousarray(outs, dtype=np.uint32).reshape(-1)

    def _outs_taken(self, outs) -> bool:
        return all(0 < int(x) <= self.m for x in outs)

    def _outs_block(self, where: str, proofs, commitments, outs, uncompressed: bool):
        """_block for a ragged block: containers of the shapes outs_shapes names, outs[i] encoded commitments per proof
        -> (raw u8, cm u8, outs u32, count)"""
        raw, cm, o = _flat_bytes(proofs), _flat_bytes(commitments), self._outs(outs)
        if self._outs_taken(o):
            version = 2 if uncompressed else 1
            need = sum(proof_bytes(self.arith, self.n, int(x), version) for x in outs_shapes(o, self.m))
            if len(raw) != need:
                raise RuntimeError("%s: %d bytes of proofs, the shapes of outs need %d" % (where, len(raw), need))
            if len(cm) != int(o.sum()) * (uncompressed_bytes(self.arith) if uncompressed else compressed_bytes(self.arith)):
                raise RuntimeError("%s: outs[i] commitments per proof" % where)
        return raw, cm, o, len(o)

    def prover_serialized_outs_workspace_bytes(self, outs) -> int:
        """bytes of device workspace prove_serialized_outputs_device needs (0: a count is not taken)"""
        o = self._outs(outs)
        return _lib.lib().bpp_prover_serialized_outs_workspace_bytes(self.handle, _some(o), len(o))

    def prove_serialized_outputs_device(self, d_values: int, d_gammas: int, outs, d_out_proofs: int, d_out_commitments: int,
                                        d_workspace: int, workspace_bytes: int, stream: int = 0, transcript: bool = False,
                                        uncompressed: bool = False, blind_key: bytes = None, index_base: int = 0,
                                        d_blinding: int = 0, amount64: bool = False):
        """prove_serialized_mixed_device over a ragged block: proof i has outs[i] values and gammas (any count 1..m) at
        d_values / d_gammas, sum(outs) in all, and gets the container of shape (n, outs_shapes(outs)[i]) and outs[i] encoded
        commitments: the two inputs of verify_serialized_outputs_device"""
        o = self._outs(outs)
        check(_lib.lib().bpp_range_prove_batch_serialized_outs_device(
            self.handle, d_values, d_gammas, _some(o), len(o), _flags(transcript, uncompressed, amount64), blind_key,
            ctypes.c_uint64(index_base), d_blinding or None,
            d_out_proofs, d_out_commitments, d_workspace, workspace_bytes, stream or None),
            "bpp_range_prove_batch_serialized_outs_device")

    def prove_serialized_outputs(self, values, gammas, transcript: bool = False, blind_key: bytes = None, index_base: int = 0,
                                 uncompressed: bool = False, amount64: bool = False):
        """values[i], gammas[i]: the values and gammas of proof i, ANY number 1..m of them -> (proofs, commitments, outs):
        proof i is the proof of shape (n, M), M = 2^ceil(log2 outs[i]), over its values and gammas padded with zeros; the
        containers back to back, outs[i] encoded commitments per proof back to back (the padded ones are the identity and
        are not written) -- what verify_serialized_outputs takes"""
        _prover_key(blind_key, transcript)
        vals, gm, outs = self._mixed_inputs(values, gammas)
        count, version = len(outs), 2 if uncompressed else 1
        pb = uncompressed_bytes(self.arith) if uncompressed else compressed_bytes(self.arith)
        taken = self._outs_taken(outs) and pb
        nbytes = sum(proof_bytes(self.arith, self.n, int(x), version) for x in outs_shapes(outs, self.m)) if taken else 0
        raw = np.zeros(max(nbytes, 1), dtype=np.uint8)
        cm = np.zeros(max(int(outs.sum()) * pb, 1), dtype=np.uint8)
        check(_lib.lib().bpp_range_prove_batch_serialized_outs(
            self.handle, _some(vals), _some(gm), _some(outs), count, _flags(transcript, uncompressed, amount64), blind_key,
            ctypes.c_uint64(index_base), _ptr(raw), _ptr(cm)), "bpp_range_prove_batch_serialized_outs")
        return raw[:nbytes].tobytes(), cm[:int(outs.sum()) * pb].tobytes(), outs

    def serialized_outs_workspace_bytes(self, outs, group: int = None) -> int:
        """bytes of device workspace verify_serialized_outputs_device needs, with `group` for its grouped form (0: a count
        or the group is not taken)"""
        o = self._outs(outs)
        if group is None:
            return _lib.lib().bpp_verifier_serialized_outs_workspace_bytes(self.handle, _some(o), len(o))
        return _lib.lib().bpp_verifier_serialized_grouped_outs_workspace_bytes(self.handle, _some(o), len(o), group)

    def verify_serialized_outputs_device(self, d_proofs: int, d_commitments: int, outs, d_ok: int, d_workspace: int,
                                         workspace_bytes: int, stream: int = 0, transcript: bool = False,
                                         uncompressed: bool = False, group: int = None, weight_key: bytes = None,
                                         index_base: int = 0):
        """verify_serialized_mixed_device over a ragged block: container i of the shape outs_shapes names, outs[i] encoded
        commitments per proof; the padded commitments are the identity and are neither read nor decompressed.  group given:
        the grouped check behind the same front (weight_key, index_base as verify_serialized_grouped_mixed_device;
        synchronises the stream) -> (groups that failed, proofs re-verified exactly), else None"""
        o = self._outs(outs)
        if group is None:
            check(_lib.lib().bpp_range_verify_batch_serialized_outs_device(
                self.handle, d_proofs, d_commitments, _some(o), len(o), _flags(transcript, uncompressed),
                d_ok, d_workspace, workspace_bytes, stream or None), "bpp_range_verify_batch_serialized_outs_device")
            return None
        stats = (ctypes.c_uint64 * 2)()
        check(_lib.lib().bpp_range_verify_batch_serialized_grouped_outs_device(
            self.handle, d_proofs, d_commitments, _some(o), len(o), _flags(transcript, uncompressed),
            _weight_key_arg(weight_key, 0), ctypes.c_uint64(index_base), group, d_ok, stats, d_workspace, workspace_bytes,
            stream or None), "bpp_range_verify_batch_serialized_grouped_outs_device")
        return int(stats[0]), int(stats[1])

    def verify_serialized_outputs(self, proofs, commitments, outs, transcript: bool = False, uncompressed: bool = False,
                                  group: int = None) -> np.ndarray:
        """proofs: the containers back to back; commitments: outs[i] encoded points per proof back to back; outs: the
        output count of each proof -> status (count,) u32: 0 Ok / 1 VerificationError / 2 FormatError.  group given: through
        the grouped check (the device form between copies, under a fresh weight key)"""
        raw, cm, o, count = self._outs_block("verify_serialized_outputs", proofs, commitments, outs, uncompressed)
        ok = np.zeros(count, dtype=np.uint32)
        if group is None:
            check(_lib.lib().bpp_range_verify_batch_serialized_outs(
                self.handle, _some(raw), _some(cm), _some(o), count, _flags(transcript, uncompressed), _some(ok)),
                "bpp_range_verify_batch_serialized_outs")
            return ok
        if count == 0:
            return ok
        import torch
        wsb = self.serialized_outs_workspace_bytes(o, group)
        if not wsb:
            check(_lib.lib().bpp_outs_shapes(_some(o), count, self.m, _some(np.zeros(count, dtype=np.uint32))), "bpp_outs_shapes")
            raise RuntimeError("verify_serialized_outputs: group must be a power of two, at least 2")
        dev = torch.device("cuda", self.arith.device)
        d_raw = torch.from_numpy(raw.copy()).to(dev)
        d_cm = torch.from_numpy(cm.copy()).to(dev)
        d_ok = torch.zeros(count, dtype=torch.int32, device=dev)
        d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        self.verify_serialized_outputs_device(d_raw.data_ptr(), d_cm.data_ptr(), o, d_ok.data_ptr(), d_ws.data_ptr(), wsb,
                                              transcript=transcript, uncompressed=uncompressed, group=group)
        torch.cuda.synchronize(dev)
        return d_ok.cpu().numpy().astype(np.uint32)

    def verify_find_outputs_outs_workspace_bytes(self, outs, n_keys: int) -> int:
        """bytes of device workspace verify_find_outputs_serialized_outs_keys_device needs (0: a count is not taken, or
        n_keys x sum(outs) is over the bound)"""
        o = self._outs(outs)
        return _lib.lib().bpp_verify_find_outputs_outs_workspace_bytes(self.handle, _some(o), len(o), n_keys)

    def verify_find_outputs_serialized_outs_keys_device(self, d_proofs: int, d_commitments: int, outs, d_keys: int, n_keys: int,
                                                        d_sealed: int, d_tags: int, d_ok: int, d_hits: int, max_hits: int,
                                                        d_n_hits: int, d_workspace: int, workspace_bytes: int, stream: int = 0,
                                                        uncompressed: bool = False, amount64: bool = False, index_base: int = 0,
                                                        d_index: int = 0, d_n_candidates: int = 0):
        """verify_find_outputs_serialized_mixed_keys_device over a ragged block: d_sealed, d_tags per REAL output
        (sum(outs) of each), output numbers in the hit records count real outputs only"""
        o = self._outs(outs)
        check(_lib.lib().bpp_range_verify_find_outputs_serialized_outs_keys_device(
            self.handle, d_proofs, d_commitments, _some(o), len(o), _flags(True, uncompressed, amount64), d_keys or None, n_keys,
            ctypes.c_uint64(index_base), d_index or None, d_sealed or None, d_tags or None, d_ok or None, d_hits or None, max_hits,
            d_n_hits or None, d_n_candidates or None, d_workspace, workspace_bytes, stream or None),
            "bpp_range_verify_find_outputs_serialized_outs_keys_device")

    def verify_find_outputs_serialized_outs_keys(self, proofs, commitments, outs, keys=(), sealed=(), tags=(),
                                                 uncompressed: bool = False, amount64: bool = False, index_base: int = 0,
                                                 index=None, max_hits: int = None):
        """verify_find_outputs_serialized_mixed_keys over a ragged block: outs[i] commitments, sealed amounts and tags per
        proof, sum(outs) of each -> (ok, hits, found, n_candidates), output numbers counting real outputs only
        (bpp_range_verify_find_outputs_serialized_outs_keys)"""
        where = "verify_find_outputs_serialized_outs_keys"
        with _packed_keys(where, keys) as (kb, nk):
            raw, cm, o, count = self._outs_block(where, proofs, commitments, outs, uncompressed)
            n_out = int(o.sum())
            idx = _index_arg(index, count, where + ": one blinding index per proof")
            se, tg = _amounts_arg(sealed), _tags_arg(tags)
            if nk and (len(se) != n_out or len(tg) != n_out):
                raise RuntimeError(where + ": one sealed amount and one tag per output")
            cap = nk * n_out if max_hits is None else int(max_hits)
            ok = np.zeros(count, dtype=np.uint32)
            rec = np.zeros((cap, 12), dtype=np.uint32)
            found = np.zeros(1, dtype=np.uint32)
            cands = np.zeros(1, dtype=np.uint32)
            some = nk > 0 and count > 0
            check(_lib.lib().bpp_range_verify_find_outputs_serialized_outs_keys(
                self.handle, _some(raw), _some(cm), _some(o), count, _flags(True, uncompressed, amount64), _ptr(kb), nk,
                ctypes.c_uint64(index_base), _ptr(idx), _ptr(se) if some else None, _ptr(tg) if some else None, _some(ok),
                _some(rec), cap, _ptr(found), _ptr(cands)), "bpp_range_verify_find_outputs_serialized_outs_keys")
        n = int(found[0])
        return ok, _hits(rec, n), n, int(cands[0])


def outs_shapes(outs, m: int) -> np.ndarray:
    """bpp_outs_shapes: the aggregation size of a proof over outs[i] outputs, 2^ceil(log2 outs[i]), for an engine of
    capacity m; BppError naming i for a count of zero or above m.  Host only."""
    o = np.ascontiguousarray(outs, dtype=np.uint32).reshape(-1)
    ms = np.zeros(len(o), dtype=np.uint32)
    check(_lib.lib().bpp_outs_shapes(_some(o), len(o), m, _some(ms)), "bpp_outs_shapes")
    return ms


def shard_cuts(ms, count: int, world: int) -> np.ndarray:
    """bpp_shard_cuts: the world + 1 cuts of a batch of `count` proofs over `world` shards, shard r taking proofs
    [cuts[r], cuts[r + 1]).  ms None: a uniform batch (sharding.shard_bounds); else proof i costs ms[i] and every shard
    costs less than sum(ms) / world + max(ms)."""
    m = None if ms is None else np.ascontiguousarray(ms, dtype=np.uint32).reshape(-1)
    if m is not None and len(m) != count:
        raise ValueError("shard_cuts: one cost per proof")
    cuts = np.zeros(world + 1 if 0 < world <= 16 else 17, dtype=np.uintp)
    check(_lib.lib().bpp_shard_cuts(_some(m), count, world, _ptr(cuts)), "bpp_shard_cuts")
    return cuts.astype(np.int64)


class VerifierPool(_Shapes):
    """One batch sharded over several devices in ONE process (include/bpp_amd.h "verifier pool"): per entry of `devices`
    a context and a verifier of capacity (n, m) on that device, the batch cut by shard_cuts, the shards' passes run on a
    host thread each, verdicts in caller order.  An ordinal may repeat -- devices=(0, 0) exercises two shards on a one-GPU
    machine.  One host thread at a time."""

    def __init__(self, pk: PublicKey, n: int, m: int, window_bits: int = 13, devices=(0,)):
        self.arith = pk.arith
        self.n, self.m = n, m
        if len(pk.G_vec) != n * m or len(pk.H_vec) != n * m:
            raise AssertionError("pk must hold n*m generators")       # range/mod.rs:90-91,252-253 assert_eq
        self.handle = None
        dev = np.ascontiguousarray(list(devices), dtype=np.int32)
        h = ctypes.c_void_p()
        G = np.ascontiguousarray(pk.G_vec)
        H = np.ascontiguousarray(pk.H_vec)
        check(_lib.lib().bpp_pool_create(pk.arith.curve, _some(dev), len(dev), _ptr(pk.gh), _ptr(G),
                                         _ptr(H), n, m, window_bits, ctypes.byref(h)), "bpp_pool_create")
        self.handle = h
        self.size = _lib.lib().bpp_pool_size(h)
        self.devices = [_lib.lib().bpp_pool_device(h, r) for r in range(self.size)]

    def close(self):
        if self.handle:
            _lib.lib().bpp_pool_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def verifier(self, r: int) -> BatchVerifier:
        """shard r's verifier, borrowed: valid while the pool lives (the _device calls, set_subgroup_check)"""
        h = ctypes.c_void_p()
        check(_lib.lib().bpp_pool_verifier(self.handle, r, ctypes.byref(h)), "bpp_pool_verifier")
        return BatchVerifier._borrowed(self.arith, h, self.n, self.m, self)

    def cuts(self, ms, count: int = None) -> np.ndarray:
        """the cuts a verify call of this pool makes for a batch with aggregation sizes ms (None: uniform, `count` proofs)"""
        return shard_cuts(ms, len(ms) if ms is not None else count, self.size)

    def verify_wire_mixed(self, records, scalars, ms=None) -> np.ndarray:
        """BatchVerifier.verify_wire_mixed over the pool (bpp_pool_verify_mixed).  ms None: a uniform batch at the
        capacity shape, records (count, 3 + 2k + m, PW)."""
        pts = self._wire_records(records)
        sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 3, 4)
        count = sc.shape[0]
        if ms is None:
            m = None
            need = count * self.mixed_points(self.m)
        else:
            m = self._ms(ms)
            if len(m) != count:
                raise RuntimeError("verify_wire_mixed: one scalar triple per entry of ms")
            need = sum(self.mixed_points(int(x)) for x in m) if self._taken(m) else None
        if need is not None and pts.shape[0] != need:
            raise RuntimeError("verify_wire_mixed: %d wire points, the shapes need %d" % (pts.shape[0], need))
        ok = np.zeros(count, dtype=np.uint32)
        check(_lib.lib().bpp_pool_verify_mixed(self.handle, _ptr(pts), _ptr(sc), _ptr(m), count, _ptr(ok)),
              "bpp_pool_verify_mixed")
        return ok

    def verify_serialized_mixed(self, proofs, commitments, ms=None, transcript: bool = False, uncompressed: bool = False,
                                grouped: bool = False, weight_key: bytes = None, index_base: int = 0, group: int = 32,
                                return_stats: bool = False):
        """BatchVerifier.verify_serialized_mixed over the pool (bpp_pool_verify_serialized_mixed): status (count,) u32,
        0 Ok / 1 VerificationError / 2 FormatError.  grouped: every shard runs the grouped check over its slice, proof i
        weighted by PRF(weight_key, index_base + i) whatever the cut (weight_key None = os.urandom(32)); with
        return_stats -> (status, (groups that failed, proofs re-verified exactly)), summed over the shards -- the stats
        depend on the cut, the statuses do not."""
        raw, cm, m, count = self._block("verify_serialized_mixed", proofs, commitments, ms, uncompressed)
        ok = np.zeros(count, dtype=np.uint32)
        stats = (ctypes.c_uint64 * 2)()
        check(_lib.lib().bpp_pool_verify_serialized_mixed(
            self.handle, _some(raw), _some(cm), _some(m), count, _flags(transcript, uncompressed), 1 if grouped else 0,
            _weight_key_arg(weight_key, 0) if grouped else None, ctypes.c_uint64(index_base), group if grouped else 0,
            _some(ok), stats), "bpp_pool_verify_serialized_mixed")
        return (ok, (int(stats[0]), int(stats[1]))) if return_stats else ok

    def verify_combined(self, points, scalars, weight_key: bytes = None, index_base: int = 0) -> int:
        """The combined check of a uniform batch at the capacity shape over the pool (bpp_pool_verify_combined): every
        shard's weighted sum, one reduce on shard 0's device.  -> 0 iff the batch passes (an empty batch does)."""
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, self.mixed_points(self.m), self.arith.PW)
        sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 3, 4)
        if sc.shape[0] != pts.shape[0]:
            raise RuntimeError("verify_combined: one scalar triple per proof record")
        ok = np.ones(1, dtype=np.uint32)
        check(_lib.lib().bpp_pool_verify_combined(self.handle, _some(pts), _some(sc), pts.shape[0],
                                                  _weight_key_arg(weight_key, 0), ctypes.c_uint64(index_base), _ptr(ok)),
              "bpp_pool_verify_combined")
        return int(ok[0])


class PassGraph:
    """One pass of the batch verifier captured into a HIP graph (bpp_verifier_graph_capture): launch() replays it over the
    buffers it was captured with.  Keep the verifier alive while its graphs are."""

    def __init__(self, handle):
        self.handle = handle

    def launch(self, stream: int = 0):
        check(_lib.lib().bpp_graph_launch(self.handle, stream or None), "bpp_graph_launch")

    def close(self):
        if self.handle:
            _lib.lib().bpp_graph_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def proof_record(proof: RangeProof, commitment_vec) -> np.ndarray:
    """[A, wip.A, wip.B, L.., R.., V..] -- the per-proof point record of the batch verifier."""
    return np.concatenate([proof.points_wire(), np.asarray(commitment_vec, dtype=np.uint64)])
