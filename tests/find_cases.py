"""What the tests of the fused verify-and-find call expect, computed without the library: the pad of a sealed amount by
hashlib, and the ordered hit list of a flag array by a prefix sum."""

import hashlib
import struct

TILE = 256   # csrc/find_terms.hpp FIND_TILE: positions per compaction block
MASK64 = (1 << 64) - 1


def pad(key: bytes, idx: int) -> int:
    """the first 8 bytes, little-endian, of SHA-256(key || "bppa" || idx as u64 LE || 0 u32 || 0 u32)"""
    assert len(key) == 32
    return int.from_bytes(hashlib.sha256(key + b"bppa" + struct.pack("<QII", idx & MASK64, 0, 0)).digest()[:8], "little")


def seal(key: bytes, amounts, indices) -> list:
    """amount XOR pad(key, index): sealing, and opening"""
    return [(int(a) ^ pad(key, int(i))) & MASK64 for a, i in zip(amounts, indices)]


def compact(flags, max_hits: int):
    """-> (number of set flags, the positions of the first max_hits of them in ascending order), by a prefix sum"""
    before, out = 0, []
    for pos, f in enumerate(flags):
        if f:
            if before < max_hits:
                out.append(pos)
            before += 1
    return before, out
