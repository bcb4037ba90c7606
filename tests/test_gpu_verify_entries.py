"""-m gpu: each of the verifier's 19 C entries once on a valid batch, then with every defect that is harmless if its
check were lost -- an unknown flag bit, group = 3, a workspace one byte short, count = 0 over guard-filled outputs, the
combined check's empty batch -- against the literal table of tests/test_verify_args_cpu.py (TABLE: what the entry itself
answers; LIVE: what the implementation behind it answers).  Such a call either runs the valid batch or is refused one layer
further in; null pointers, count bounds and a missing weight source stay on the CPU, where a lost check reads nothing.
And every size getter against the bytes the library returned before the entries' checks became data (GETTERS).

One BLS12-381 and one edwards25519 engine at (n, m) = (8, 2); three proofs (valid, a flipped scalar, valid); the mixed
entries take m_of = [1, 2, 2]."""

import ctypes

import numpy as np
import pytest

import oracle as O
import pyref as P
import verdict_corpus as VC
from gpu_util import need_gpu
from test_verify_args_cpu import TABLE, expected

pytestmark = pytest.mark.gpu

N, M, WB, COUNT = 8, 2, 5, 3
M_OF = (1, 2, 2)
GUARD = 7
STATS_GUARD = 0x5a5a5a5a5a5a5a5a

# bytes per getter, recorded on the library as it was at a1134c0: {curve: {"getter(arguments)": bytes}}
GETTERS = {
    "bls12_381": {
        "bpp_verifier_partial_bytes()": 160, "bpp_verifier_workspace_bytes(0)": 0,
        "bpp_verifier_combined_workspace_bytes(0)": 2048, "bpp_verifier_serialized_workspace_bytes(0)": 0,
        "bpp_verifier_mixed_workspace_bytes(0)": 0, "bpp_verifier_serialized_mixed_workspace_bytes(0)": 0,
        "bpp_verifier_grouped_workspace_bytes(0, 2)": 78592, "bpp_verifier_serialized_grouped_workspace_bytes(0, 2)": 78592,
        "bpp_verifier_grouped_mixed_workspace_bytes(0, 2)": 1024,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(0, 2)": 1024,
        "bpp_verifier_grouped_workspace_bytes(0, 4)": 78592, "bpp_verifier_serialized_grouped_workspace_bytes(0, 4)": 78592,
        "bpp_verifier_grouped_mixed_workspace_bytes(0, 4)": 1024,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(0, 4)": 1024, "bpp_verifier_workspace_bytes(1)": 76032,
        "bpp_verifier_combined_workspace_bytes(1)": 47104, "bpp_verifier_serialized_workspace_bytes(1)": 78336,
        "bpp_verifier_mixed_workspace_bytes(1)": 72960, "bpp_verifier_serialized_mixed_workspace_bytes(1)": 72960,
        "bpp_verifier_grouped_workspace_bytes(1, 2)": 201728, "bpp_verifier_serialized_grouped_workspace_bytes(1, 2)": 204032,
        "bpp_verifier_grouped_mixed_workspace_bytes(1, 2)": 192512,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(1, 2)": 192768,
        "bpp_verifier_grouped_workspace_bytes(1, 4)": 201728, "bpp_verifier_serialized_grouped_workspace_bytes(1, 4)": 204032,
        "bpp_verifier_grouped_mixed_workspace_bytes(1, 4)": 192512,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(1, 4)": 192768, "bpp_verifier_workspace_bytes(3)": 224512,
        "bpp_verifier_combined_workspace_bytes(3)": 114432, "bpp_verifier_serialized_workspace_bytes(3)": 230144,
        "bpp_verifier_mixed_workspace_bytes(3)": 156416, "bpp_verifier_serialized_mixed_workspace_bytes(3)": 156160,
        "bpp_verifier_grouped_workspace_bytes(3, 2)": 506112, "bpp_verifier_serialized_grouped_workspace_bytes(3, 2)": 511744,
        "bpp_verifier_grouped_mixed_workspace_bytes(3, 2)": 414464,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(3, 2)": 414720,
        "bpp_verifier_grouped_workspace_bytes(3, 4)": 430336, "bpp_verifier_serialized_grouped_workspace_bytes(3, 4)": 435968,
        "bpp_verifier_grouped_mixed_workspace_bytes(3, 4)": 338688,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(3, 4)": 338944, "bpp_verifier_workspace_bytes(2049)": 152430848,
        "bpp_verifier_combined_workspace_bytes(2049)": 74135552, "bpp_verifier_serialized_workspace_bytes(2049)": 155865600,
        "bpp_verifier_mixed_workspace_bytes(2049)": 105099776, "bpp_verifier_serialized_mixed_workspace_bytes(2049)": 104862208,
        "bpp_verifier_grouped_workspace_bytes(2049, 2)": 312598784,
        "bpp_verifier_serialized_grouped_workspace_bytes(2049, 2)": 316033536,
        "bpp_verifier_grouped_mixed_workspace_bytes(2049, 2)": 249172736,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(2049, 2)": 249148416,
        "bpp_verifier_grouped_workspace_bytes(2049, 4)": 273735936,
        "bpp_verifier_serialized_grouped_workspace_bytes(2049, 4)": 277170688,
        "bpp_verifier_grouped_mixed_workspace_bytes(2049, 4)": 210309888,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(2049, 4)": 210285568,
        "bpp_verifier_grouped_workspace_bytes(3, 0)": 0, "bpp_verifier_serialized_grouped_workspace_bytes(3, 0)": 0,
        "bpp_verifier_grouped_mixed_workspace_bytes(3, 0)": 0, "bpp_verifier_grouped_workspace_bytes(3, 1)": 0,
        "bpp_verifier_serialized_grouped_workspace_bytes(3, 1)": 0, "bpp_verifier_grouped_mixed_workspace_bytes(3, 1)": 0,
        "bpp_verifier_grouped_workspace_bytes(3, 3)": 0, "bpp_verifier_serialized_grouped_workspace_bytes(3, 3)": 0,
        "bpp_verifier_grouped_mixed_workspace_bytes(3, 3)": 0, "bpp_verifier_mixed_workspace_bytes(null, 3)": 0,
        "bpp_verifier_serialized_mixed_workspace_bytes(3, count 2^25)": 0,
    },
    "ed25519": {
        "bpp_verifier_partial_bytes()": 144, "bpp_verifier_workspace_bytes(0)": 0,
        "bpp_verifier_combined_workspace_bytes(0)": 1792, "bpp_verifier_serialized_workspace_bytes(0)": 0,
        "bpp_verifier_mixed_workspace_bytes(0)": 0, "bpp_verifier_serialized_mixed_workspace_bytes(0)": 0,
        "bpp_verifier_grouped_workspace_bytes(0, 2)": 65024, "bpp_verifier_serialized_grouped_workspace_bytes(0, 2)": 65024,
        "bpp_verifier_grouped_mixed_workspace_bytes(0, 2)": 1024,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(0, 2)": 1024,
        "bpp_verifier_grouped_workspace_bytes(0, 4)": 65024, "bpp_verifier_serialized_grouped_workspace_bytes(0, 4)": 65024,
        "bpp_verifier_grouped_mixed_workspace_bytes(0, 4)": 1024,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(0, 4)": 1024, "bpp_verifier_workspace_bytes(1)": 62976,
        "bpp_verifier_combined_workspace_bytes(1)": 37632, "bpp_verifier_serialized_workspace_bytes(1)": 64768,
        "bpp_verifier_mixed_workspace_bytes(1)": 60928, "bpp_verifier_serialized_mixed_workspace_bytes(1)": 60928,
        "bpp_verifier_grouped_workspace_bytes(1, 2)": 165888, "bpp_verifier_serialized_grouped_workspace_bytes(1, 2)": 167680,
        "bpp_verifier_grouped_mixed_workspace_bytes(1, 2)": 159232,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(1, 2)": 159488,
        "bpp_verifier_grouped_workspace_bytes(1, 4)": 165888, "bpp_verifier_serialized_grouped_workspace_bytes(1, 4)": 167680,
        "bpp_verifier_grouped_mixed_workspace_bytes(1, 4)": 159232,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(1, 4)": 159488, "bpp_verifier_workspace_bytes(3)": 186368,
        "bpp_verifier_combined_workspace_bytes(3)": 89344, "bpp_verifier_serialized_workspace_bytes(3)": 190720,
        "bpp_verifier_mixed_workspace_bytes(3)": 129280, "bpp_verifier_serialized_mixed_workspace_bytes(3)": 129280,
        "bpp_verifier_grouped_workspace_bytes(3, 2)": 414720, "bpp_verifier_serialized_grouped_workspace_bytes(3, 2)": 419072,
        "bpp_verifier_grouped_mixed_workspace_bytes(3, 2)": 340992,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(3, 2)": 341248,
        "bpp_verifier_grouped_workspace_bytes(3, 4)": 351744, "bpp_verifier_serialized_grouped_workspace_bytes(3, 4)": 356096,
        "bpp_verifier_grouped_mixed_workspace_bytes(3, 4)": 278016,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(3, 4)": 278272, "bpp_verifier_workspace_bytes(2049)": 126498304,
        "bpp_verifier_combined_workspace_bytes(2049)": 57463552, "bpp_verifier_serialized_workspace_bytes(2049)": 129080576,
        "bpp_verifier_mixed_workspace_bytes(2049)": 86958848, "bpp_verifier_serialized_mixed_workspace_bytes(2049)": 86786816,
        "bpp_verifier_grouped_workspace_bytes(2049, 2)": 255576576,
        "bpp_verifier_serialized_grouped_workspace_bytes(2049, 2)": 258158848,
        "bpp_verifier_grouped_mixed_workspace_bytes(2049, 2)": 204540672,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(2049, 2)": 204516352,
        "bpp_verifier_grouped_workspace_bytes(2049, 4)": 223193600,
        "bpp_verifier_serialized_grouped_workspace_bytes(2049, 4)": 225775872,
        "bpp_verifier_grouped_mixed_workspace_bytes(2049, 4)": 172157696,
        "bpp_verifier_serialized_grouped_mixed_workspace_bytes(2049, 4)": 172133376,
        "bpp_verifier_grouped_workspace_bytes(3, 0)": 0, "bpp_verifier_serialized_grouped_workspace_bytes(3, 0)": 0,
        "bpp_verifier_grouped_mixed_workspace_bytes(3, 0)": 0, "bpp_verifier_grouped_workspace_bytes(3, 1)": 0,
        "bpp_verifier_serialized_grouped_workspace_bytes(3, 1)": 0, "bpp_verifier_grouped_mixed_workspace_bytes(3, 1)": 0,
        "bpp_verifier_grouped_workspace_bytes(3, 3)": 0, "bpp_verifier_serialized_grouped_workspace_bytes(3, 3)": 0,
        "bpp_verifier_grouped_mixed_workspace_bytes(3, 3)": 0, "bpp_verifier_mixed_workspace_bytes(null, 3)": 0,
        "bpp_verifier_serialized_mixed_workspace_bytes(3, count 2^25)": 0,
    },
}


def getter_rows(L, h):
    """every size getter of the verifier family at counts 0, 1, 3, 2 049 and groups 2, 4 -> {"getter(arguments)": bytes}"""
    rows = {"bpp_verifier_partial_bytes()": L.bpp_verifier_partial_bytes(h)}
    for count in (0, 1, 3, 2049):
        m_of = (ctypes.c_uint32 * max(count, 1))(*[M_OF[i % 3] for i in range(count)])
        for name in ("bpp_verifier_workspace_bytes", "bpp_verifier_combined_workspace_bytes",
                     "bpp_verifier_serialized_workspace_bytes"):
            rows["%s(%d)" % (name, count)] = getattr(L, name)(h, count)
        for name in ("bpp_verifier_mixed_workspace_bytes", "bpp_verifier_serialized_mixed_workspace_bytes"):
            rows["%s(%d)" % (name, count)] = getattr(L, name)(h, m_of, count)
        for group in (2, 4):
            for name in ("bpp_verifier_grouped_workspace_bytes", "bpp_verifier_serialized_grouped_workspace_bytes"):
                rows["%s(%d, %d)" % (name, count, group)] = getattr(L, name)(h, count, group)
            for name in ("bpp_verifier_grouped_mixed_workspace_bytes",
                         "bpp_verifier_serialized_grouped_mixed_workspace_bytes"):
                rows["%s(%d, %d)" % (name, count, group)] = getattr(L, name)(h, m_of, count, group)
    # what the getters refuse: a group that is no power of two at least 2, a null m_of, a count beyond one launch
    for group in (0, 1, 3):
        rows["bpp_verifier_grouped_workspace_bytes(3, %d)" % group] = L.bpp_verifier_grouped_workspace_bytes(h, 3, group)
        rows["bpp_verifier_serialized_grouped_workspace_bytes(3, %d)" % group] = \
            L.bpp_verifier_serialized_grouped_workspace_bytes(h, 3, group)
        rows["bpp_verifier_grouped_mixed_workspace_bytes(3, %d)" % group] = \
            L.bpp_verifier_grouped_mixed_workspace_bytes(h, (ctypes.c_uint32 * 3)(*M_OF), 3, group)
    rows["bpp_verifier_mixed_workspace_bytes(null, 3)"] = L.bpp_verifier_mixed_workspace_bytes(h, None, 3)
    rows["bpp_verifier_serialized_mixed_workspace_bytes(3, count 2^25)"] = \
        L.bpp_verifier_serialized_mixed_workspace_bytes(h, (ctypes.c_uint32 * 3)(*M_OF), 1 << 25)
    return rows


class Batch:
    """the inputs of every entry on the device and on the host, and guard-filled outputs"""

    def __init__(self, torch, B, cname):
        from bulletproofsplus_amd import _lib
        self.torch, self.L, self.dev = torch, _lib.lib(), torch.device("cuda:0")
        cps = {m: VC.corpus(cname, N, m) for m in (1, 2)}
        cap = cps[M]
        self.arith = B.Arith(cname)
        self.bv = B.BatchVerifier(B.PublicKey.from_points(self.arith, cap.gh, cap.G, cap.H), N, M, window_bits=WB)
        self.h = self.bv.handle
        fixed = [(cap, cap.by_name(nm)) for nm in ("valid_1", "flip_s", "valid_2")]
        mixed = [(cps[1], cps[1].by_name("valid_1")), (cap, cap.by_name("flip_s")), (cap, cap.by_name("valid_2"))]
        assert [c.expect for _, c in fixed] == [0, 1, 0] and [c.status for _, c in fixed] == [0, 1, 0]
        self.want = [0, 1, 0]                      # wire and serialized, fixed and mixed alike
        self.k = cap.k
        self.host, self.d = {}, {}
        for tag, cases in (("", fixed), ("_mixed", mixed)):
            recs = np.concatenate([np.concatenate([c.pts, c.V]) for _, c in cases])
            enc = [VC.encode_case(cp, c) for cp, c in cases]
            self.host["points" + tag] = np.ascontiguousarray(recs)
            self.host["scalars" + tag] = np.ascontiguousarray(np.stack([c.sc for _, c in cases]))
            self.host["proofs" + tag] = np.frombuffer(b"".join(b for b, _ in enc), np.uint8).copy()
            self.host["commitments" + tag] = np.frombuffer(b"".join(m for _, m in enc), np.uint8).copy()
        self.host["records"] = np.frombuffer(b"".join(
            P.compress_point(cap.curve, Pt) for _, c in fixed
            for Pt in O.wire_to_points(cap.cid, VC.canonical_inf(cap, np.concatenate([c.pts, c.V])))), np.uint8).copy()
        for name, arr in self.host.items():
            self.d[name] = torch.from_numpy(arr.view(np.int64) if arr.dtype == np.uint64 else arr).to(self.dev)
        self.m_of = (ctypes.c_uint32 * COUNT)(*M_OF)
        self.key = bytes(range(32))
        self.d_ok = torch.empty(COUNT, dtype=torch.int32, device=self.dev)
        self.h_ok = np.empty(COUNT, dtype=np.uint32)
        self.d_ch = torch.empty(COUNT * (3 + self.k) * 4, dtype=torch.int64, device=self.dev)
        self.d_partial = torch.empty(self.L.bpp_verifier_partial_bytes(self.h), dtype=self.torch.uint8, device=self.dev)
        self.stats = (ctypes.c_uint64 * 2)()
        self.graph = ctypes.c_void_p()
        self.ws = {}

    def workspace(self, getter, *args):
        """-> (device pointer, the getter's bytes) for a batch of 3; one buffer per getter"""
        m_of = (self.m_of,) if "mixed" in getter else ()
        wsb = getattr(self.L, getter)(self.h, *m_of, COUNT, *args)
        assert wsb > 0, getter
        if getter not in self.ws:
            self.ws[getter] = self.torch.empty(wsb + 256, dtype=self.torch.uint8, device=self.dev)
        return self.ws[getter].data_ptr(), wsb

    def reset(self):
        self.d_ok.fill_(GUARD)
        self.h_ok.fill(GUARD)
        self.d_ch.fill_(GUARD)
        self.stats[0] = self.stats[1] = STATS_GUARD
        self.torch.cuda.synchronize()

    def close(self):
        if self.graph:
            self.L.bpp_graph_destroy(self.graph)
        self.bv.close()


def _p(t):
    return t.data_ptr()


def _hp(a):
    return a.ctypes.data


# entry -> (call(b, count, flags, group, short) -> rc, which outputs it writes: "d_ok" / "h_ok" / "d_ch" / "combined", its
# workspace getter and the getter's trailing arguments, has a flags argument, a group, stats); short: bytes taken off the
# workspace size
def _entries():
    def ws(b, getter, short, *args):
        p, wsb = b.workspace(getter, *args)
        return p, wsb - short

    def run(b, count, flags, group, short):
        p, w = ws(b, "bpp_verifier_workspace_bytes", short)
        return b.L.bpp_verifier_run(b.h, _p(b.d["points"]), _p(b.d["scalars"]), count, None, _p(b.d_ok), p, w, None, None, None)

    def graph_capture(b, count, flags, group, short):
        p, w = ws(b, "bpp_verifier_workspace_bytes", short)
        return b.L.bpp_verifier_graph_capture(b.h, _p(b.d["points"]), _p(b.d["scalars"]), count, None, _p(b.d_ok), p, w,
                                              ctypes.byref(b.graph))

    def run_combined(b, count, flags, group, short):
        p, w = ws(b, "bpp_verifier_combined_workspace_bytes", short)
        return b.L.bpp_verifier_run_combined(b.h, _p(b.d["points"]), _p(b.d["scalars"]), count, None, b.key, 0, None,
                                             _p(b.d_partial), _p(b.d_ok), p, w, None)

    def run_grouped(b, count, flags, group, short):
        p, w = ws(b, "bpp_verifier_grouped_workspace_bytes", short, 4)
        return b.L.bpp_verifier_run_grouped(b.h, _p(b.d["points"]), _p(b.d["scalars"]), count, None, b.key, 0, None, group,
                                            _p(b.d_ok), b.stats, p, w, None)

    def grouped_begin(b, count, flags, group, short):
        p, w = ws(b, "bpp_verifier_grouped_workspace_bytes", short, 4)
        return b.L.bpp_verifier_grouped_begin(b.h, _p(b.d["points"]), _p(b.d["scalars"]), count, None, b.key, 0, None, group,
                                              _p(b.d_ok), p, w, None)

    def grouped_finish(b, count, flags, group, short):
        p, w = ws(b, "bpp_verifier_grouped_workspace_bytes", short, 4)
        if count and group == 4 and not short:      # the valid call completes a pass begun on the same buffers
            rc = b.L.bpp_verifier_grouped_begin(b.h, _p(b.d["points"]), _p(b.d["scalars"]), count, None, b.key, 0, None,
                                                group, _p(b.d_ok), p, w, None)
            assert rc == 0
        return b.L.bpp_verifier_grouped_finish(b.h, _p(b.d["points"]), _p(b.d["scalars"]), count, None, group, _p(b.d_ok),
                                               b.stats, p, w, None)

    def derive_challenges(b, count, flags, group, short):
        return b.L.bpp_verifier_derive_challenges(b.h, _p(b.d["points"]), count, _p(b.d_ch), None)

    def run_mixed(b, count, flags, group, short):
        p, w = ws(b, "bpp_verifier_mixed_workspace_bytes", short)
        return b.L.bpp_verifier_run_mixed(b.h, _p(b.d["points_mixed"]), _p(b.d["scalars_mixed"]), b.m_of, count, None,
                                          _p(b.d_ok), p, w, None, None)

    def derive_challenges_mixed(b, count, flags, group, short):
        p, w = ws(b, "bpp_verifier_mixed_workspace_bytes", short)
        return b.L.bpp_verifier_derive_challenges_mixed(b.h, _p(b.d["points_mixed"]), b.m_of, count, _p(b.d_ch), p, w, None)

    def ser_device(b, count, flags, group, short):
        p, w = ws(b, "bpp_verifier_serialized_workspace_bytes", short)
        return b.L.bpp_range_verify_batch_serialized_device(b.h, _p(b.d["proofs"]), _p(b.d["commitments"]), count, flags,
                                                            _p(b.d_ok), p, w, None)

    def ser_grouped_device(b, count, flags, group, short):
        p, w = ws(b, "bpp_verifier_serialized_grouped_workspace_bytes", short, 4)
        return b.L.bpp_range_verify_batch_serialized_grouped_device(b.h, _p(b.d["proofs"]), _p(b.d["commitments"]), count,
                                                                    flags, b.key, 0, group, _p(b.d_ok), b.stats, p, w, None)

    def ser_mixed_device(b, count, flags, group, short):
        p, w = ws(b, "bpp_verifier_serialized_mixed_workspace_bytes", short)
        return b.L.bpp_range_verify_batch_serialized_mixed_device(b.h, _p(b.d["proofs_mixed"]), _p(b.d["commitments_mixed"]),
                                                                  b.m_of, count, flags, _p(b.d_ok), p, w, None)

    def run_grouped_mixed(b, count, flags, group, short):
        p, w = ws(b, "bpp_verifier_grouped_mixed_workspace_bytes", short, 4)
        return b.L.bpp_verifier_run_grouped_mixed(b.h, _p(b.d["points_mixed"]), _p(b.d["scalars_mixed"]), b.m_of, count, None,
                                                  b.key, 0, None, group, _p(b.d_ok), b.stats, p, w, None)

    def ser_grouped_mixed_device(b, count, flags, group, short):
        p, w = ws(b, "bpp_verifier_serialized_grouped_mixed_workspace_bytes", short, 4)
        return b.L.bpp_range_verify_batch_serialized_grouped_mixed_device(
            b.h, _p(b.d["proofs_mixed"]), _p(b.d["commitments_mixed"]), b.m_of, count, flags, b.key, 0, group, _p(b.d_ok),
            b.stats, p, w, None)

    def verify_batch(b, count, flags, group, short):
        return b.L.bpp_range_verify_batch(b.h, _hp(b.host["points"]), _hp(b.host["scalars"]), count, _hp(b.h_ok))

    def verify_batch_mixed(b, count, flags, group, short):
        return b.L.bpp_range_verify_batch_mixed(b.h, _hp(b.host["points_mixed"]), _hp(b.host["scalars_mixed"]), b.m_of, count,
                                                _hp(b.h_ok))

    def verify_batch_compressed(b, count, flags, group, short):
        return b.L.bpp_range_verify_batch_compressed(b.h, _hp(b.host["records"]), _hp(b.host["scalars"]), count, _hp(b.h_ok))

    def verify_batch_serialized(b, count, flags, group, short):
        return b.L.bpp_range_verify_batch_serialized(b.h, _hp(b.host["proofs"]), _hp(b.host["commitments"]), count, flags,
                                                     _hp(b.h_ok))

    def verify_batch_serialized_mixed(b, count, flags, group, short):
        return b.L.bpp_range_verify_batch_serialized_mixed(b.h, _hp(b.host["proofs_mixed"]), _hp(b.host["commitments_mixed"]),
                                                           b.m_of, count, flags, _hp(b.h_ok))

    #        entry: (call, output, has a workspace, flags, group, stats)
    return {
        "bpp_verifier_run": (run, "d_ok", 1, 0, 0, 0),
        "bpp_verifier_graph_capture": (graph_capture, "d_ok", 1, 0, 0, 0),
        "bpp_verifier_run_combined": (run_combined, "combined", 1, 0, 0, 0),
        "bpp_verifier_run_grouped": (run_grouped, "d_ok", 1, 0, 1, 1),
        "bpp_verifier_grouped_begin": (grouped_begin, None, 1, 0, 1, 0),
        "bpp_verifier_grouped_finish": (grouped_finish, "d_ok", 1, 0, 1, 1),
        "bpp_verifier_derive_challenges": (derive_challenges, "d_ch", 0, 0, 0, 0),
        "bpp_verifier_run_mixed": (run_mixed, "d_ok", 1, 0, 0, 0),
        "bpp_verifier_derive_challenges_mixed": (derive_challenges_mixed, "d_ch", 1, 0, 0, 0),
        "bpp_range_verify_batch_serialized_device": (ser_device, "d_ok", 1, 1, 0, 0),
        "bpp_range_verify_batch_serialized_grouped_device": (ser_grouped_device, "d_ok", 1, 1, 1, 1),
        "bpp_range_verify_batch_serialized_mixed_device": (ser_mixed_device, "d_ok", 1, 1, 0, 0),
        "bpp_verifier_run_grouped_mixed": (run_grouped_mixed, "d_ok", 1, 0, 1, 1),
        "bpp_range_verify_batch_serialized_grouped_mixed_device": (ser_grouped_mixed_device, "d_ok", 1, 1, 1, 1),
        "bpp_range_verify_batch": (verify_batch, "h_ok", 0, 0, 0, 0),
        "bpp_range_verify_batch_mixed": (verify_batch_mixed, "h_ok", 0, 0, 0, 0),
        "bpp_range_verify_batch_compressed": (verify_batch_compressed, "h_ok", 0, 0, 0, 0),
        "bpp_range_verify_batch_serialized": (verify_batch_serialized, "h_ok", 0, 1, 0, 0),
        "bpp_range_verify_batch_serialized_mixed": (verify_batch_serialized_mixed, "h_ok", 0, 1, 0, 0),
    }


ENTRIES = _entries()


def _outcome(b, rc, stats):
    """the call's answer in TABLE's words"""
    out = str(rc) if rc >= 0 else "%d %s" % (rc, b.L.bpp_last_error().decode())
    if stats:
        zeroed = (b.stats[0], b.stats[1]) == (0, 0)
        assert zeroed or (b.stats[0], b.stats[1]) == (STATS_GUARD, STATS_GUARD), tuple(b.stats)
        out += " | stats zeroed" if zeroed else " | stats kept"
    return out


def _untouched(b):
    b.torch.cuda.synchronize()
    return (b.d_ok.cpu().numpy() == GUARD).all() and (b.h_ok == GUARD).all() and (b.d_ch.cpu().numpy() == GUARD).all()


@pytest.mark.parametrize("cname", ["bls12_381", "ed25519"])
def test_every_verifier_entry_valid_and_refused(cname):
    torch = need_gpu()
    import bulletproofsplus_amd as B
    assert set(ENTRIES) == set(TABLE)
    b = Batch(torch, B, cname)
    try:
        got = getter_rows(b.L, b.h)
        assert got == GETTERS[cname], {k: (got.get(k), v) for k, v in GETTERS[cname].items() if got.get(k) != v}
        for entry, (call, output, has_ws, has_flags, has_group, has_stats) in ENTRIES.items():
            # the valid batch
            b.reset()
            rc = call(b, COUNT, 0, 4, 0)
            torch.cuda.synchronize()
            assert rc == 0, (entry, rc, b.L.bpp_last_error())
            if output == "d_ok":
                assert b.d_ok.cpu().numpy().tolist() == b.want, entry
            elif output == "h_ok":
                assert b.h_ok.tolist() == b.want, entry
            elif output == "combined":
                assert b.d_ok.cpu().numpy().tolist()[0] == 1, entry      # one proof of the batch is invalid
            elif output == "d_ch":
                assert not (b.d_ch.cpu().numpy() == GUARD).all(), entry
            if has_stats:
                assert (b.stats[0], b.stats[1]) == (1, COUNT), (entry, tuple(b.stats))   # one group of 4 holds all three
            # the harmless defects
            defects = [("count:0", (0, 0, 4, 0))]
            if has_flags:
                defects.append(("flag:0x4", (COUNT, 4, 4, 0)))
            if has_group:
                defects.append(("group:3", (COUNT, 0, 3, 0)))
            if has_ws:
                defects.append(("ws:short", (COUNT, 0, 4, 1)))
            for defect, args in defects:
                want = expected(entry, defect)
                assert want is not None, (entry, defect)
                b.reset()
                got = _outcome(b, call(b, *args), has_stats)
                assert got == want, (entry, defect, got, want)
                if defect == "count:0" or defect == "flag:0x4":
                    assert _untouched(b), (entry, defect)
                torch.cuda.synchronize()
    finally:
        b.close()
