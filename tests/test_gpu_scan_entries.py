"""-m gpu: each of the receiver's 14 C entries -- mask recovery, the one-key scan, the many-key scan and the four
verify-and-find calls, device and host each -- once on a valid block, then with every defect that is harmless if its check
were lost: count = 0 over guard-filled outputs, an unknown flag bit, a missing BPP_SER_TRANSCRIPT (the literal table of
tests/test_scan_args_cpu.py: what the entry itself answers), and what the implementation BEHIND the entry refuses on a live
engine (LIVE below): an m_i above the engine's, a workspace one byte short, container version 2 on edwards25519.  Such a
call is refused on the host before any launch; null pointers and the count bounds stay on the CPU, where a lost check reads
nothing.  (n or m above 255 and log2(n m) > 14 are refused behind the entry too, but no engine of such a shape can be
created: VS_MAXM = 64 and n <= 64.)  And every size getter of the family against the bytes the library returned before the
entries' checks became one (GETTERS).

One BLS12-381 and one edwards25519 engine at (n, m) = (8, 4); four proofs with m_of = [1, 2, 4, 1] -- three aggregation
classes -- over eight outputs of two scanning keys and a foreign one.  Expected values never come from the entry under test:
the masks are output_cases.mask's, Gamma of the aggregated proofs is the checker's algebra on the wire records of the same
proofs, pads and tags are hashlib's; the Python wrappers (the host entries) are checked against those, and every entry,
called through ctypes, against the wrappers word for word."""

import ctypes
import hashlib

import numpy as np
import pytest

import find_cases as FC
import oracle as O
import output_cases as OC
import recover_cases as RC
import tag_cases as TC
import test_gpu_find as TF
import test_gpu_outputs as TO
import test_gpu_recover as TR
from gpu_util import need_gpu
from test_scan_args_cpu import TABLE, expected

pytestmark = pytest.mark.gpu

N, BASE, GUARD = TR.N, TR.BASE, 0x5a5a5a5a
K0, K1 = (hashlib.sha256(b"scan entries: scanning key %d" % q).digest() for q in range(2))
FOREIGN = hashlib.sha256(b"scan entries: a key nobody scans with").digest()
KEYS = [K1, K0]                 # K0 is also the key of the one-key calls, and made the aggregated proofs
MS = [1, 2, 4, 1]
COUNT, N_OUT = len(MS), sum(MS)
FIRST = [sum(MS[:i]) for i in range(COUNT)]
PROOF_OF = [i for i, m in enumerate(MS) for _ in range(m)]
PLACE_OF = [j for m in MS for j in range(m)]
INDEX = [BASE + i for i in range(COUNT)]
OWNER = [K0, K1, FOREIGN, K0, K1, FOREIGN, K0, K1]
MAKER = [K0, K0, K0, K1]        # a single output is proved under its owner's key: rewinding gives the mask it was given
MAX_HITS = 6
FS, V2 = 1, 2                   # BPP_SER_TRANSCRIPT, BPP_SER_UNCOMPRESSED

# What a LIVE engine answers where TABLE says "run" and the implementation behind the entry refuses: read from mixed.hpp
# (mixed_plan), outs_plan.hpp (outs_shapes), impl_verify.hpp (container_args_ok) and the "workspace too small" behind each
# layout in recover.hpp, recover_keys.hpp and find.hpp at c2f4b69.
LIVE = {
    "m:above": "-1 m_of[1] = 8: not a power of two in [1, 4]",
    "outs:above": "-1 outs_of[1] = 5: not in [1, 4]",
    "ws:short": "-1 workspace too small",
    "ed25519:v2": "-1 container version 2 (uncompressed points) is not offered for this curve",
}

# bytes per getter (its name without bpp_ and _workspace_bytes), recorded on the library as it was at c2f4b69:
# {curve: {"getter(count or m_of[, n_keys])": bytes}}
GETTERS = {
    "bls12_381": {
        "recover_mixed(0)": 0, "recover_mixed(1)": 256, "recover_mixed(4)": 256, "recover_mixed(2049)": 33024,
        "recover_mixed(null, 4)": 0, "recover_mixed([1, 3, 2])": 0, "recover_mixed([1, 0, 2])": 0, "recover_mixed([1, 8, 2])": 0,
        "recover_mixed([1, 129, 2])": 0, "recover_mixed(4, count 2^25)": 0, "scan_serialized_mixed(0)": 0,
        "scan_serialized_mixed(1)": 3072, "scan_serialized_mixed(4)": 8192, "scan_serialized_mixed(2049)": 3427328,
        "scan_serialized_mixed(null, 4)": 0, "scan_serialized_mixed([1, 3, 2])": 0, "scan_serialized_mixed([1, 0, 2])": 0,
        "scan_serialized_mixed([1, 8, 2])": 0, "scan_serialized_mixed([1, 129, 2])": 0, "scan_serialized_mixed(4, count 2^25)": 0,
        "scan_serialized_mixed_keys(0, 0)": 0, "scan_serialized_mixed_keys(0, 1)": 0, "scan_serialized_mixed_keys(0, 3)": 0,
        "scan_serialized_mixed_keys(1, 0)": 3328, "scan_serialized_mixed_keys(1, 1)": 3328,
        "scan_serialized_mixed_keys(1, 3)": 3328, "scan_serialized_mixed_keys(4, 0)": 10240,
        "scan_serialized_mixed_keys(4, 1)": 10240, "scan_serialized_mixed_keys(4, 3)": 10240,
        "scan_serialized_mixed_keys(2049, 0)": 4492544, "scan_serialized_mixed_keys(2049, 1)": 4492544,
        "scan_serialized_mixed_keys(2049, 3)": 4492544, "scan_serialized_mixed_keys(null, 4, 1)": 0,
        "scan_serialized_mixed_keys([1, 3, 2], 1)": 0, "scan_serialized_mixed_keys([1, 0, 2], 1)": 0,
        "scan_serialized_mixed_keys([1, 8, 2], 1)": 0, "scan_serialized_mixed_keys([1, 129, 2], 1)": 0,
        "scan_serialized_mixed_keys(4, count 2^25, 1)": 0, "scan_serialized_mixed_keys(4, 8388608)": 0,
        "scan_serialized_mixed_keys(4, 4611686018427387904)": 0, "verify_find_serialized_mixed_keys(0, 0)": 0,
        "verify_find_serialized_mixed_keys(0, 1)": 0, "verify_find_serialized_mixed_keys(0, 3)": 0,
        "verify_find_serialized_mixed_keys(1, 0)": 73728, "verify_find_serialized_mixed_keys(1, 1)": 74752,
        "verify_find_serialized_mixed_keys(1, 3)": 74752, "verify_find_serialized_mixed_keys(4, 0)": 147712,
        "verify_find_serialized_mixed_keys(4, 1)": 148736, "verify_find_serialized_mixed_keys(4, 3)": 148992,
        "verify_find_serialized_mixed_keys(2049, 0)": 74289152, "verify_find_serialized_mixed_keys(2049, 1)": 74380288,
        "verify_find_serialized_mixed_keys(2049, 3)": 74560512, "verify_find_serialized_mixed_keys(null, 4, 1)": 0,
        "verify_find_serialized_mixed_keys([1, 3, 2], 1)": 0, "verify_find_serialized_mixed_keys([1, 0, 2], 1)": 0,
        "verify_find_serialized_mixed_keys([1, 8, 2], 1)": 0, "verify_find_serialized_mixed_keys([1, 129, 2], 1)": 0,
        "verify_find_serialized_mixed_keys(4, count 2^25, 1)": 0, "verify_find_serialized_mixed_keys(4, 8388608)": 0,
        "verify_find_serialized_mixed_keys(4, 4611686018427387904)": 0, "verify_find_tagged(0, 0)": 256,
        "verify_find_tagged(0, 1)": 256, "verify_find_tagged(0, 3)": 256, "verify_find_tagged(1, 0)": 73984,
        "verify_find_tagged(1, 1)": 75776, "verify_find_tagged(1, 3)": 75776, "verify_find_tagged(4, 0)": 147968,
        "verify_find_tagged(4, 1)": 149760, "verify_find_tagged(4, 3)": 150016, "verify_find_tagged(2049, 0)": 74289408,
        "verify_find_tagged(2049, 1)": 74385408, "verify_find_tagged(2049, 3)": 74574080, "verify_find_tagged(null, 4, 1)": 0,
        "verify_find_tagged([1, 3, 2], 1)": 0, "verify_find_tagged([1, 0, 2], 1)": 0, "verify_find_tagged([1, 8, 2], 1)": 0,
        "verify_find_tagged([1, 129, 2], 1)": 0, "verify_find_tagged(4, count 2^25, 1)": 0, "verify_find_tagged(4, 8388608)": 0,
        "verify_find_tagged(4, 4611686018427387904)": 0, "verify_find_outputs(0, 0)": 256, "verify_find_outputs(0, 1)": 256,
        "verify_find_outputs(0, 3)": 256, "verify_find_outputs(1, 0)": 73216, "verify_find_outputs(1, 1)": 75008,
        "verify_find_outputs(1, 3)": 75008, "verify_find_outputs(4, 0)": 146688, "verify_find_outputs(4, 1)": 148480,
        "verify_find_outputs(4, 3)": 148992, "verify_find_outputs(2049, 0)": 73793024, "verify_find_outputs(2049, 1)": 73982976,
        "verify_find_outputs(2049, 3)": 74360320, "verify_find_outputs(null, 4, 1)": 0, "verify_find_outputs([1, 3, 2], 1)": 0,
        "verify_find_outputs([1, 0, 2], 1)": 0, "verify_find_outputs([1, 8, 2], 1)": 0, "verify_find_outputs([1, 129, 2], 1)": 0,
        "verify_find_outputs(4, count 2^25, 1)": 0, "verify_find_outputs(4, 8388608)": 0,
        "verify_find_outputs(4, 4611686018427387904)": 0, "verify_find_outputs_outs(0, 0)": 256,
        "verify_find_outputs_outs(0, 1)": 256, "verify_find_outputs_outs(0, 3)": 256, "verify_find_outputs_outs(1, 0)": 73216,
        "verify_find_outputs_outs(1, 1)": 75008, "verify_find_outputs_outs(1, 3)": 75008,
        "verify_find_outputs_outs(4, 0)": 146688, "verify_find_outputs_outs(4, 1)": 148480,
        "verify_find_outputs_outs(4, 3)": 148992, "verify_find_outputs_outs(2049, 0)": 73793024,
        "verify_find_outputs_outs(2049, 1)": 73982976, "verify_find_outputs_outs(2049, 3)": 74360320,
        "verify_find_outputs_outs(null, 4, 1)": 0, "verify_find_outputs_outs([1, 3, 2], 1)": 92416,
        "verify_find_outputs_outs([1, 0, 2], 1)": 0, "verify_find_outputs_outs([1, 8, 2], 1)": 0,
        "verify_find_outputs_outs([1, 129, 2], 1)": 0, "verify_find_outputs_outs(4, count 2^25, 1)": 0,
        "verify_find_outputs_outs(4, 8388608)": 0, "verify_find_outputs_outs(4, 4611686018427387904)": 0,
    },
    "ed25519": {
        "recover_mixed(0)": 0, "recover_mixed(1)": 256, "recover_mixed(4)": 256, "recover_mixed(2049)": 33024,
        "recover_mixed(null, 4)": 0, "recover_mixed([1, 3, 2])": 0, "recover_mixed([1, 0, 2])": 0, "recover_mixed([1, 8, 2])": 0,
        "recover_mixed([1, 129, 2])": 0, "recover_mixed(4, count 2^25)": 0, "scan_serialized_mixed(0)": 0,
        "scan_serialized_mixed(1)": 2560, "scan_serialized_mixed(4)": 6656, "scan_serialized_mixed(2049)": 2607616,
        "scan_serialized_mixed(null, 4)": 0, "scan_serialized_mixed([1, 3, 2])": 0, "scan_serialized_mixed([1, 0, 2])": 0,
        "scan_serialized_mixed([1, 8, 2])": 0, "scan_serialized_mixed([1, 129, 2])": 0, "scan_serialized_mixed(4, count 2^25)": 0,
        "scan_serialized_mixed_keys(0, 0)": 0, "scan_serialized_mixed_keys(0, 1)": 0, "scan_serialized_mixed_keys(0, 3)": 0,
        "scan_serialized_mixed_keys(1, 0)": 2816, "scan_serialized_mixed_keys(1, 1)": 2816,
        "scan_serialized_mixed_keys(1, 3)": 2816, "scan_serialized_mixed_keys(4, 0)": 8704,
        "scan_serialized_mixed_keys(4, 1)": 8704, "scan_serialized_mixed_keys(4, 3)": 8704,
        "scan_serialized_mixed_keys(2049, 0)": 3672832, "scan_serialized_mixed_keys(2049, 1)": 3672832,
        "scan_serialized_mixed_keys(2049, 3)": 3672832, "scan_serialized_mixed_keys(null, 4, 1)": 0,
        "scan_serialized_mixed_keys([1, 3, 2], 1)": 0, "scan_serialized_mixed_keys([1, 0, 2], 1)": 0,
        "scan_serialized_mixed_keys([1, 8, 2], 1)": 0, "scan_serialized_mixed_keys([1, 129, 2], 1)": 0,
        "scan_serialized_mixed_keys(4, count 2^25, 1)": 0, "scan_serialized_mixed_keys(4, 8388608)": 0,
        "scan_serialized_mixed_keys(4, 4611686018427387904)": 0, "verify_find_serialized_mixed_keys(0, 0)": 0,
        "verify_find_serialized_mixed_keys(0, 1)": 0, "verify_find_serialized_mixed_keys(0, 3)": 0,
        "verify_find_serialized_mixed_keys(1, 0)": 61696, "verify_find_serialized_mixed_keys(1, 1)": 62720,
        "verify_find_serialized_mixed_keys(1, 3)": 62720, "verify_find_serialized_mixed_keys(4, 0)": 123136,
        "verify_find_serialized_mixed_keys(4, 1)": 124160, "verify_find_serialized_mixed_keys(4, 3)": 124416,
        "verify_find_serialized_mixed_keys(2049, 0)": 62071040, "verify_find_serialized_mixed_keys(2049, 1)": 62162176,
        "verify_find_serialized_mixed_keys(2049, 3)": 62342400, "verify_find_serialized_mixed_keys(null, 4, 1)": 0,
        "verify_find_serialized_mixed_keys([1, 3, 2], 1)": 0, "verify_find_serialized_mixed_keys([1, 0, 2], 1)": 0,
        "verify_find_serialized_mixed_keys([1, 8, 2], 1)": 0, "verify_find_serialized_mixed_keys([1, 129, 2], 1)": 0,
        "verify_find_serialized_mixed_keys(4, count 2^25, 1)": 0, "verify_find_serialized_mixed_keys(4, 8388608)": 0,
        "verify_find_serialized_mixed_keys(4, 4611686018427387904)": 0, "verify_find_tagged(0, 0)": 256,
        "verify_find_tagged(0, 1)": 256, "verify_find_tagged(0, 3)": 256, "verify_find_tagged(1, 0)": 61952,
        "verify_find_tagged(1, 1)": 63744, "verify_find_tagged(1, 3)": 63744, "verify_find_tagged(4, 0)": 123392,
        "verify_find_tagged(4, 1)": 125184, "verify_find_tagged(4, 3)": 125440, "verify_find_tagged(2049, 0)": 62071296,
        "verify_find_tagged(2049, 1)": 62167296, "verify_find_tagged(2049, 3)": 62355968, "verify_find_tagged(null, 4, 1)": 0,
        "verify_find_tagged([1, 3, 2], 1)": 0, "verify_find_tagged([1, 0, 2], 1)": 0, "verify_find_tagged([1, 8, 2], 1)": 0,
        "verify_find_tagged([1, 129, 2], 1)": 0, "verify_find_tagged(4, count 2^25, 1)": 0, "verify_find_tagged(4, 8388608)": 0,
        "verify_find_tagged(4, 4611686018427387904)": 0, "verify_find_outputs(0, 0)": 256, "verify_find_outputs(0, 1)": 256,
        "verify_find_outputs(0, 3)": 256, "verify_find_outputs(1, 0)": 61184, "verify_find_outputs(1, 1)": 62976,
        "verify_find_outputs(1, 3)": 62976, "verify_find_outputs(4, 0)": 122112, "verify_find_outputs(4, 1)": 123904,
        "verify_find_outputs(4, 3)": 124416, "verify_find_outputs(2049, 0)": 61574912, "verify_find_outputs(2049, 1)": 61764864,
        "verify_find_outputs(2049, 3)": 62142208, "verify_find_outputs(null, 4, 1)": 0, "verify_find_outputs([1, 3, 2], 1)": 0,
        "verify_find_outputs([1, 0, 2], 1)": 0, "verify_find_outputs([1, 8, 2], 1)": 0, "verify_find_outputs([1, 129, 2], 1)": 0,
        "verify_find_outputs(4, count 2^25, 1)": 0, "verify_find_outputs(4, 8388608)": 0,
        "verify_find_outputs(4, 4611686018427387904)": 0, "verify_find_outputs_outs(0, 0)": 256,
        "verify_find_outputs_outs(0, 1)": 256, "verify_find_outputs_outs(0, 3)": 256, "verify_find_outputs_outs(1, 0)": 61184,
        "verify_find_outputs_outs(1, 1)": 62976, "verify_find_outputs_outs(1, 3)": 62976,
        "verify_find_outputs_outs(4, 0)": 122112, "verify_find_outputs_outs(4, 1)": 123904,
        "verify_find_outputs_outs(4, 3)": 124416, "verify_find_outputs_outs(2049, 0)": 61574912,
        "verify_find_outputs_outs(2049, 1)": 61764864, "verify_find_outputs_outs(2049, 3)": 62142208,
        "verify_find_outputs_outs(null, 4, 1)": 0, "verify_find_outputs_outs([1, 3, 2], 1)": 76032,
        "verify_find_outputs_outs([1, 0, 2], 1)": 0, "verify_find_outputs_outs([1, 8, 2], 1)": 0,
        "verify_find_outputs_outs([1, 129, 2], 1)": 0, "verify_find_outputs_outs(4, count 2^25, 1)": 0,
        "verify_find_outputs_outs(4, 8388608)": 0, "verify_find_outputs_outs(4, 4611686018427387904)": 0,
    },
}

_GETTERS = (
    ("bpp_recover_mixed_workspace_bytes", False), ("bpp_scan_serialized_mixed_workspace_bytes", False),
    ("bpp_scan_serialized_mixed_keys_workspace_bytes", True), ("bpp_verify_find_serialized_mixed_keys_workspace_bytes", True),
    ("bpp_verify_find_tagged_workspace_bytes", True), ("bpp_verify_find_outputs_workspace_bytes", True),
    ("bpp_verify_find_outputs_outs_workspace_bytes", True),
)


def getter_rows(L, h):
    """every size getter of the receiver's family at counts 0, 1, 4, 2 049 and 0, 1, 3 keys, and what they refuse
    -> {"getter(arguments)": bytes}"""
    rows = {}

    def units(values):
        return (ctypes.c_uint32 * max(len(values), 1))(*values)

    def put(tag, name, keyed, u, count, n_keys):
        short = name.replace("bpp_", "").replace("_workspace_bytes", "")
        rows["%s(%s%s)" % (short, tag, ", %d" % n_keys if keyed else "")] = getattr(L, name)(h, u, count, *((n_keys,) if keyed else ()))

    for name, keyed in _GETTERS:
        for count in (0, 1, 4, 2049):
            for n_keys in (0, 1, 3) if keyed else (0,):
                put(str(count), name, keyed, units([MS[i % COUNT] for i in range(count)]), count, n_keys)
        # what the getters refuse: a null array, an m_i no engine takes or above this engine's, a count or a pair count beyond
        # one launch (the array unread)
        put("null, 4", name, keyed, None, 4, 1)
        put("[1, 3, 2]", name, keyed, units([1, 3, 2]), 3, 1)
        put("[1, 0, 2]", name, keyed, units([1, 0, 2]), 3, 1)
        put("[1, 8, 2]", name, keyed, units([1, 8, 2]), 3, 1)
        put("[1, 129, 2]", name, keyed, units([1, 129, 2]), 3, 1)
        put("4, count 2^25", name, keyed, units(MS), 1 << 25, 1)
        if keyed:
            put("4", name, keyed, units(MS), 4, 1 << 23)
            put("4", name, keyed, units(MS), 4, 1 << 62)
    return rows


def _ints(words, rows):
    """rows x 4 u64 of canonical scalars -> ints"""
    return [int(x) for x in O.wire_to_scalars(np.ascontiguousarray(words).view(np.uint64).reshape(-1, 4)[:rows].copy())]


class Block:
    """the inputs of every entry on the device and on the host, guard-filled outputs, and what must come out"""

    def __init__(self, torch, cname):
        from bulletproofsplus_amd import _lib
        self.torch, self.L, self.dev = torch, _lib.lib(), torch.device("cuda:0")
        r = RC.ORDER[cname]
        self.B, self.a, self.bv = TR._engine(cname)
        bv = self.bv
        self.h = bv.handle
        self.amounts = [17 + 13 * o for o in range(N_OUT)]
        self.masks = [OC.mask(OWNER[o], INDEX[PROOF_OF[o]], PLACE_OF[o], r) for o in range(N_OUT)]
        pr, cs, recs, scs, self.gamma = [], [], [], [], []
        for i, m in enumerate(MS):
            o = FIRST[i]
            kw = dict(transcript=True, blind_key=MAKER[i], index_base=INDEX[i])
            raw, cm, _ = bv.prove_serialized_mixed([self.amounts[o:o + m]], [self.masks[o:o + m]], **kw)
            rec, sc = bv.prove_batch_mixed([self.amounts[o:o + m]], [self.masks[o:o + m]], **kw)
            pr.append(bytes(raw))
            cs.append(bytes(cm))
            recs.append(np.asarray(rec[0]))
            scs.append(np.asarray(sc[0], dtype=np.uint64).reshape(3, 4))
            z = TR._checker_challenges(cname, N, m, recs[i], scs[i])[1] if m > 1 else 0
            self.gamma.append(RC.gamma_of(r, self.masks[o:o + m], z))
        assert self.gamma[0] == self.masks[0] and self.gamma[3] == self.masks[7]
        self.raw, self.cm = b"".join(pr), b"".join(cs)
        self.d_ch, ch = TR._derive(torch, bv, MS, recs)
        self.cand = [self.amounts[FIRST[i]] for i in range(COUNT)]
        self.psealed = [self.amounts[FIRST[i]] ^ FC.pad(OWNER[FIRST[i]], INDEX[i]) for i in range(COUNT)]
        self.ptags = [TC.tag(OWNER[FIRST[i]], INDEX[i]) for i in range(COUNT)]
        self.osealed = [self.amounts[o] ^ OC.pad(OWNER[o], INDEX[PROOF_OF[o]], PLACE_OF[o]) for o in range(N_OUT)]
        self.otags = [OC.tag(OWNER[o], INDEX[PROOF_OF[o]], PLACE_OF[o]) for o in range(N_OUT)]
        self.rewound = [(0, 3, self.amounts[7], self.masks[7]), (1, 0, self.amounts[0], self.masks[0])]
        self.listed = [(q, o, self.amounts[o], self.masks[o]) for q, k in enumerate(KEYS) for o in range(N_OUT) if OWNER[o] == k]
        self.n_cand = {"tagged": len(TC.candidates(KEYS, INDEX, self.ptags, [m == 1 for m in MS])),
                       "outputs": len(TO._candidates(KEYS, INDEX, MS, self.otags, [0] * COUNT))}
        assert len(self.listed) == 6 and self.n_cand["tagged"] >= 2 and self.n_cand["outputs"] >= 6
        self.host = {
            "proofs": np.frombuffer(self.raw, np.uint8).copy(), "commitments": np.frombuffer(self.cm, np.uint8).copy(),
            "scalars": np.ascontiguousarray(np.stack(scs)), "challenges": np.ascontiguousarray(np.concatenate([O.scalars_to_wire(c) for c in ch])),
            "keys": np.frombuffer(b"".join(KEYS), np.uint8).copy(), "cand": np.array(self.cand, dtype=np.uint64),
            "cand_keys": np.array(self.cand * len(KEYS), dtype=np.uint64), "psealed": np.array(self.psealed, dtype=np.uint64),
            "ptags": np.array(self.ptags, dtype=np.uint8), "osealed": np.array(self.osealed, dtype=np.uint64),
            "otags": np.array(self.otags, dtype=np.uint8),
        }
        self.d = {name: TR._dev(torch, arr) for name, arr in self.host.items()}
        self.m_of = (ctypes.c_uint32 * COUNT)(*MS)
        # outputs: Gamma (key-major, 4 u64 each), status, verdicts, hit records, [n_hits, guard, n_candidates, guard]
        shapes = {"masks": len(KEYS) * COUNT * 8, "status": len(KEYS) * COUNT, "ok": COUNT, "hits": (MAX_HITS + 1) * 12, "n": 4}
        self.h_out = {k: np.empty(n, dtype=np.uint32) for k, n in shapes.items()}
        self.d_out = {k: torch.empty(n, dtype=torch.int32, device=self.dev) for k, n in shapes.items()}
        self.ws = {}

    def workspace(self, getter, n_keys=None):
        """-> (device pointer, the getter's bytes) for the valid block; one buffer per getter"""
        wsb = getattr(self.L, getter)(self.h, self.m_of, COUNT, *(() if n_keys is None else (n_keys,)))
        assert wsb > 0, getter
        if getter not in self.ws:
            self.ws[getter] = self.torch.empty(wsb + 256, dtype=self.torch.uint8, device=self.dev)
        return self.ws[getter].data_ptr(), wsb

    def reset(self):
        for t in self.d_out.values():
            t.fill_(GUARD)
        for arr in self.h_out.values():
            arr.fill(GUARD)
        self.torch.cuda.synchronize()

    def out(self, device):
        """-> {name: u32 words} of the outputs an entry of that side wrote"""
        self.torch.cuda.synchronize()
        if not device:
            return {k: v.copy() for k, v in self.h_out.items()}
        return {k: t.cpu().numpy().view(np.uint32) for k, t in self.d_out.items()}

    def close(self):
        self.bv.close()


def _entries():
    """entry -> (call(b, units, count, flags, short) -> rc, family, device); units: m_of, or outs_of for the ragged entries;
    short: bytes taken off the workspace size"""
    def side(b, device):
        src, out = (b.d, b.d_out) if device else (b.host, b.h_out)
        p = (lambda t: t.data_ptr()) if device else (lambda a: a.ctypes.data)
        return (lambda name: p(src[name])), (lambda name, words=0: p(out[name]) + 4 * words)

    def recover(device):
        def call(b, units, count, flags, short):
            i, o = side(b, device)
            head = (b.h, i("scalars"), units, count, b.d_ch.data_ptr() if device else i("challenges"), K0, BASE, None, None, o("masks"))
            if not device:
                return b.L.bpp_range_recover_masks_mixed(*head)
            p, w = b.workspace("bpp_recover_mixed_workspace_bytes")
            return b.L.bpp_range_recover_masks_mixed_device(*head, p, w - short, None)
        return call

    def scan(device):
        def call(b, units, count, flags, short):
            i, o = side(b, device)
            head = (b.h, i("proofs"), i("commitments"), units, count, flags, K0, BASE, None, None, i("cand"), o("masks"), o("status"))
            if not device:
                return b.L.bpp_range_scan_serialized_mixed(*head)
            p, w = b.workspace("bpp_scan_serialized_mixed_workspace_bytes")
            return b.L.bpp_range_scan_serialized_mixed_device(*head, p, w - short, None)
        return call

    def scan_keys(device):
        def call(b, units, count, flags, short):
            i, o = side(b, device)
            head = (b.h, i("proofs"), i("commitments"), units, count, flags, i("keys"), len(KEYS), BASE, None, i("cand_keys"),
                    o("masks"), o("status"))
            if not device:
                return b.L.bpp_range_scan_serialized_mixed_keys(*head)
            p, w = b.workspace("bpp_scan_serialized_mixed_keys_workspace_bytes", len(KEYS))
            return b.L.bpp_range_scan_serialized_mixed_keys_device(*head, p, w - short, None)
        return call

    def find(device, tagged):
        def call(b, units, count, flags, short):
            i, o = side(b, device)
            head = (b.h, i("proofs"), i("commitments"), units, count, flags | 0x200, i("keys"), len(KEYS), BASE, None, i("psealed"),
                    o("ok"), o("hits"), MAX_HITS, o("n"))
            tail = (i("ptags"), o("n", 2)) if tagged else ()
            name = "bpp_range_verify_find_tagged_serialized_mixed_keys" if tagged else "bpp_range_verify_find_serialized_mixed_keys"
            if not device:
                return getattr(b.L, name)(*head, *tail)
            p, w = b.workspace("bpp_verify_find_tagged_workspace_bytes" if tagged
                               else "bpp_verify_find_serialized_mixed_keys_workspace_bytes", len(KEYS))
            return getattr(b.L, name + "_device")(*head, *tail, p, w - short, None)
        return call

    def find_outputs(device, ragged):
        def call(b, units, count, flags, short):
            i, o = side(b, device)
            head = (b.h, i("proofs"), i("commitments"), units, count, flags, i("keys"), len(KEYS), BASE, None, i("osealed"),
                    i("otags"), o("ok"), o("hits"), MAX_HITS, o("n"), o("n", 2))
            name = "bpp_range_verify_find_outputs_serialized_%s_keys" % ("outs" if ragged else "mixed")
            if not device:
                return getattr(b.L, name)(*head)
            p, w = b.workspace("bpp_verify_find_outputs_outs_workspace_bytes" if ragged else "bpp_verify_find_outputs_workspace_bytes",
                               len(KEYS))
            return getattr(b.L, name + "_device")(*head, p, w - short, None)
        return call

    out = {}
    for device in (True, False):
        d = "_device" if device else ""
        out["bpp_range_recover_masks_mixed" + d] = (recover(device), "recover", device)
        out["bpp_range_scan_serialized_mixed" + d] = (scan(device), "scan", device)
        out["bpp_range_scan_serialized_mixed_keys" + d] = (scan_keys(device), "keys", device)
        out["bpp_range_verify_find_serialized_mixed_keys" + d] = (find(device, False), "untagged", device)
        out["bpp_range_verify_find_tagged_serialized_mixed_keys" + d] = (find(device, True), "tagged", device)
        out["bpp_range_verify_find_outputs_serialized_mixed_keys" + d] = (find_outputs(device, False), "outputs", device)
        out["bpp_range_verify_find_outputs_serialized_outs_keys" + d] = (find_outputs(device, True), "outs", device)
    return out


ENTRIES = _entries()


def _wrappers(b):
    """the block through the Python wrappers, each checked against what the test made -> {family: what an entry of the
    family must write, in words}"""
    bv, raw, cm = b.bv, b.raw, b.cm
    g = b.gamma
    rec = bv.recover_masks(b.host["scalars"], MS, b.host["challenges"], blind_key=K0, index_base=BASE)
    assert rec[:3] == g[:3] and rec[3] not in (0, g[3])        # proof 3 was made under K1
    st, got = bv.scan_serialized_mixed(raw, cm, MS, transcript=True, blind_key=K0, index_base=BASE, amounts=b.cand)
    assert st.tolist() == [0, 3, 3, 1] and got == g[:3] + [0]
    kst, kgot = bv.scan_serialized_mixed_keys(raw, cm, MS, KEYS, index_base=BASE, amounts=[b.cand] * len(KEYS))
    assert kst.tolist() == [[1, 3, 3, 0], [0, 3, 3, 1]] and kgot[1] == got
    assert kgot[0][0] == 0 and kgot[0][3] == g[3] and kgot[0][1] not in (0, g[1]) and kgot[0][2] not in (0, g[2])
    want = {"recover": dict(masks=rec), "scan": dict(masks=got, status=st.tolist()),
            "keys": dict(masks=kgot[0] + kgot[1], status=kst.reshape(-1).tolist())}
    finds = {
        "untagged": bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, amounts=b.psealed, sealed=True, index_base=BASE,
                                                         max_hits=MAX_HITS) + (None,),
        "tagged": bv.verify_find_serialized_mixed_keys(raw, cm, MS, KEYS, amounts=b.psealed, sealed=True, index_base=BASE,
                                                       max_hits=MAX_HITS, tags=b.ptags),
        "outputs": bv.verify_find_outputs_serialized_mixed_keys(raw, cm, MS, KEYS, b.osealed, b.otags, index_base=BASE,
                                                                max_hits=MAX_HITS),
        "outs": bv.verify_find_outputs_serialized_outs_keys(raw, cm, MS, KEYS, b.osealed, b.otags, index_base=BASE,
                                                            max_hits=MAX_HITS),
    }
    for family, (ok, hits, found, n_cand) in finds.items():
        hit_list = b.rewound if family in ("untagged", "tagged") else b.listed
        assert ok.tolist() == [0] * COUNT and hits == hit_list and found == len(hit_list), family
        assert n_cand == b.n_cand.get("outputs" if family == "outs" else family), family
        want[family] = dict(ok=[0] * COUNT, hits=TF._records(hits), n_hits=found, n_cand=n_cand)
    return want


def _check_valid(entry, family, got, want):
    """the words a valid call wrote against the wrappers' of its family; everything behind them is still the guard"""
    if "masks" in want:
        rows = len(want["masks"])
        assert _ints(got["masks"], rows) == want["masks"] and (got["masks"][rows * 8:] == GUARD).all(), entry
        status = want.get("status", [])
        assert got["status"][:len(status)].tolist() == status and (got["status"][len(status):] == GUARD).all(), entry
        assert all((got[k] == GUARD).all() for k in ("ok", "hits", "n")), entry
        return
    n = want["n_hits"]
    assert got["ok"].tolist() == want["ok"], entry
    assert got["hits"].reshape(-1, 12)[:n].tolist() == want["hits"] and (got["hits"][n * 12:] == GUARD).all(), entry
    assert got["n"].tolist() == [n, GUARD, GUARD if want["n_cand"] is None else want["n_cand"], GUARD], entry
    assert (got["masks"] == GUARD).all() and (got["status"] == GUARD).all(), entry


@pytest.mark.parametrize("cname", ["bls12_381", "ed25519"])
def test_every_receiver_entry_valid_and_refused(cname):
    torch = need_gpu()
    assert set(ENTRIES) == set(TABLE)
    b = Block(torch, cname)
    try:
        rows = getter_rows(b.L, b.h)
        assert rows == GETTERS[cname], {k: (rows.get(k), v) for k, v in GETTERS[cname].items() if rows.get(k) != v}
        want = _wrappers(b)
        above = {False: (ctypes.c_uint32 * COUNT)(1, 8, 4, 1), True: (ctypes.c_uint32 * COUNT)(1, 5, 4, 1)}
        for entry, (call, family, device) in ENTRIES.items():
            ragged, has_flags = family == "outs", family != "recover"
            # the valid block
            b.reset()
            rc = call(b, b.m_of, COUNT, FS, 0)
            assert rc == 0, (entry, rc, b.L.bpp_last_error())
            _check_valid(entry, family, b.out(device), want[family])
            # the harmless defects: (defect, units, count, flags, short) -> TABLE's answer, or LIVE's
            defects = [("count:0", b.m_of, 0, FS, 0, expected(entry, "count:0")),
                       ("outs:above" if ragged else "m:above", above[ragged], COUNT, FS, 0, LIVE["outs:above" if ragged else "m:above"])]
            if has_flags:
                defects.append(("flag:0x4", b.m_of, COUNT, FS | 4, 0, expected(entry, "flag:0x4")))
                defects.append(("nofs", b.m_of, COUNT, 0, 0, expected(entry, "nofs")))
                if cname == "ed25519":
                    defects.append(("ed25519:v2", b.m_of, COUNT, FS | V2, 0, LIVE["ed25519:v2"]))
            if device:
                defects.append(("ws:short", b.m_of, COUNT, FS, 1, LIVE["ws:short"]))
            for defect, units, count, flags, short, answer in defects:
                b.reset()
                rc = call(b, units, count, flags, short)
                got = str(rc) if rc >= 0 else "%d %s" % (rc, b.L.bpp_last_error().decode())
                assert got == answer, (entry, defect, got, answer)
                out = b.out(device)
                if defect == "count:0" and "n_cand" in want[family]:   # a find entry: no proof, so no hit and no candidate
                    assert out.pop("n").tolist() == [0, GUARD, GUARD if family == "untagged" else 0, GUARD], entry
                assert all((words == GUARD).all() for words in out.values()), (entry, defect)
    finally:
        b.close()
