"""What the tests of the tagged verify-and-find call expect, computed without the library: the view tag of an output by
hashlib, the candidates of a block from who made each tag, and the candidate list of the tag test's tiles by a prefix
sum."""

import hashlib
import struct

import find_cases as FC

MASK64 = (1 << 64) - 1


def tag(key: bytes, idx: int) -> int:
    """the first byte of SHA-256(key || "bppt" || idx as u64 LE || 0 u32 || 0 u32)"""
    assert len(key) == 32
    return hashlib.sha256(key + b"bppt" + struct.pack("<QII", idx & MASK64, 0, 0)).digest()[0]


def tags(key: bytes, indices) -> list:
    return [tag(key, int(i)) for i in indices]


def candidates(keys, indices, tag_bytes, eligible) -> list:
    """the pairs (key number, position) whose proof is eligible (a verified single output with defined coefficients) and
    whose tag is the key's, in ascending (key number, position)"""
    return [(j, i) for j, k in enumerate(keys) for i, idx in enumerate(indices) if eligible[i] and tag(k, idx) == tag_bytes[i]]


def candidate_list(flags_by_key, max_entries=None):
    """flags_by_key[j][p]: is pair (key j, launch position p) a candidate -> (count, the pair numbers j * count + p of the
    candidates in ascending order), by a prefix sum as find_cases.compact makes it"""
    count = len(flags_by_key[0]) if flags_by_key else 0
    flat = [f for row in flags_by_key for f in row]
    n, out = FC.compact(flat, len(flat) if max_entries is None else max_entries)
    assert all(0 <= q < len(flags_by_key) * count for q in out)
    return n, out
