"""What the tests of outputs with derived masks expect, computed without the library: the mask, the pad and the tag of
output j of the proof with blinding index idx under a recipient's key, by hashlib; and the numbering of the per-output tag
test's lanes by a plain enumeration."""

import hashlib
import struct

MASK64 = (1 << 64) - 1
TILE, BLOCK, ROUNDS = 256, 64, 4   # csrc/find_terms.hpp FIND_TILE, FIND_BLOCK, FIND_ROUNDS


def _block(key: bytes, tag4: bytes, idx: int, a: int, b: int) -> bytes:
    """SHA-256(key || tag (4 ASCII bytes) || idx as u64 LE || a as u32 LE || b as u32 LE)"""
    assert len(key) == 32 and len(tag4) == 4
    return hashlib.sha256(key + tag4 + struct.pack("<QII", idx & MASK64, a, b)).digest()


def mask(key: bytes, idx: int, j: int, r: int) -> int:
    """(c0 + 2^256 c1) mod r, zero replaced by one; c_h = B("bppm", idx, j, h) as a little-endian 256-bit integer"""
    c0 = int.from_bytes(_block(key, b"bppm", idx, j, 0), "little")
    c1 = int.from_bytes(_block(key, b"bppm", idx, j, 1), "little")
    return (c0 + (c1 << 256)) % r or 1


def pad(key: bytes, idx: int, j: int) -> int:
    """the first 8 bytes of B("bppa", idx, j, 0) as a little-endian u64"""
    return int.from_bytes(_block(key, b"bppa", idx, j, 0)[:8], "little")


def tag(key: bytes, idx: int, j: int) -> int:
    """the first byte of B("bppt", idx, j, 0)"""
    return _block(key, b"bppt", idx, j, 0)[0]


def blinding_slot(key: bytes, idx: int, slot: int, r: int) -> int:
    """the prover's blinding slot of the same (idx, slot): the mask's construction under "bppb" """
    c0 = int.from_bytes(_block(key, b"bppb", idx, slot, 0), "little")
    c1 = int.from_bytes(_block(key, b"bppb", idx, slot, 1), "little")
    return (c0 + (c1 << 256)) % r or 1


def tag_lanes(n_keys: int, count_c: int, m_c: int):
    """the per-output tag test of one class, enumerated: -> [(tile, round, lane, key number, proof p, place j)] for every
    pair, tile after tile.  Each key's row of count_c * m_c launch output positions is cut into tiles of its own."""
    outs = count_c * m_c
    per_key = -(-outs // TILE)
    rows = []
    for q in range(n_keys):
        for x in range(outs):
            t, within = divmod(x, TILE)
            rows.append((q * per_key + t, within // BLOCK, within % BLOCK, q, x // m_c, x % m_c))
    return rows
