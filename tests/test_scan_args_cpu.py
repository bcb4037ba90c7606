"""CPU: the argument checks of the receiver's 14 C entries (csrc/scan_args.hpp: scan_args over ScanEntry data for mask
recovery and the scans, find_args for verify-and-find) answer every defect as the per-entry ladders of capi.hip did before
they became one check each.

tests/host/scan_args_host_test.cpp (g++, under the sanitizers with BPP_HOST_SANITIZE=1) includes the check header alone and
walks every entry over: each required pointer null, one at a time; count 0, 1, 0x7fffffff/64, one more, 2^32; n_keys 0;
n_keys x units at the pair bound and one above, a product that wraps 64 bits included; the flag bits outside the entry's set,
with and without count 0; both blinding sources, an index without a key, a blinding source without the transcript; m_of of
[1,3,2], [0,1,1], [2,4,12]; outs_of holding 0 and 129; a misaligned key pointer; a workspace of zero bytes; and the pairs of
defects whose winner the ladders' ORDER decides (null with unknown flag, null with count 0, the sealed flag with an unknown
one per output, the pair bound with a missing transcript, a bad m_i with a missing transcript or an empty workspace).  It
prints `entry, defect, outcome` per row; TABLE below is what must come out.

Every row of TABLE was derived by reading the ladder of that entry in capi.hip at commit c2f4b69 (the last one with
ladders: recover_args, scan_keys_args, find_args, find_outs_args and the statements around them), line by line, not from the
new check: "run" is a call that passes the entry's checks and goes on to the implementation, "0" one the entry answers
itself (an empty call; a find entry zeroes its counts first), "-1 text" a refusal with bpp_last_error()'s text.  The valid
call has count 3, m_of (or outs_of) [1, 2, 4], two keys (the one-key entries: a blind_key), BPP_SER_TRANSCRIPT, room for 4
hits and a workspace of 64 bytes.  Things the ladders never looked at stay "run": an m_i above the engine's, the container
version, log2(n m), a ragged block's counts and a workspace too small but not empty are refused one layer further in
(tests/test_gpu_scan_entries.py sees those on a live engine)."""

import subprocess

from test_host_arith_cpu import _build

NULL = "-1 null argument"
FLAG = "-1 unknown flag"
SHORT = "-1 workspace too small"
LAUNCH = "-1 count too large for one launch"
BOTH = "-1 blind_key and d_blinding are both given"
NOKEY = "-1 d_index is the index of a blind_key: it needs one"
NEEDS_FS = "-1 blinding needs BPP_SER_TRANSCRIPT"
VERDICTS_FS = "-1 the verdicts need BPP_SER_TRANSCRIPT"
ALIGN = "-1 d_keys must be 4-byte aligned"
PROOF_PAIRS = "-1 n_keys x count too large for one launch"
OUTPUT_PAIRS = "-1 n_keys x n_out too large for one launch"
SEALED = "-1 BPP_FIND_AMOUNTS_SEALED is not taken: amounts are always sealed here"
BAD_M = {"1,3,2": "-1 m_of[1] = 3: not a power of two", "0,1,1": "-1 m_of[0] = 0: not a power of two",
         "2,4,12": "-1 m_of[2] = 12: not a power of two"}

UNKNOWN_BITS = "flag:0x4 flag:0x400 flag:0x4+count:0 flag:0x400+count:0 null:%s+flag:0x4 null:%s+flag:0x400"
OVER_PAIRS = ("count:33554431 count:33554432 count:4294967296 pairs:over pairs:1x33554432 pairs:33554432x1 pairs:wrap "
              "nofs+pairs:over")
AT_PAIRS = "pairs:at pairs:1x33554431 pairs:33554431x1"


def _rows(device, common, device_only, host_only):
    """-> {outcome: defects} of one entry: the rows both forms share and those of its own form"""
    out = {k: v.split() for k, v in common.items()}
    for k, v in (device_only if device else host_only).items():
        out.setdefault(k, []).extend(v.split())
    return {k: " ".join(v) for k, v in out.items()}


def _recover(device):
    return _rows(device, {
        "run": "valid count:1 count:33554431 nosource",
        NULL: "null:v null:scalars null:m_of null:out_masks",
        "0": "count:0 null:scalars+count:0",
        LAUNCH: "count:33554432 count:4294967296",
        BAD_M["1,3,2"]: "m_of:1,3,2", BAD_M["0,1,1"]: "m_of:0,1,1", BAD_M["2,4,12"]: "m_of:2,4,12",
        BOTH: "both both+count:33554432",
        NOKEY: "index:nokey",
    }, {NULL: "null:ws", SHORT: "ws:0", BAD_M["1,3,2"]: "m_of:1,3,2+ws:0"}, {})


def _one_key(device):
    return _rows(device, {
        "run": "valid count:1 count:33554431 nosource nofs+nosource",
        NULL: "null:v null:proofs null:commitments null:m_of null:out_masks null:status",
        "0": "count:0 null:proofs+count:0",
        LAUNCH: "count:33554432 count:4294967296 nofs+count:33554432",
        FLAG: UNKNOWN_BITS % ("proofs", "proofs") + " flag:0x200 flag:0x200+count:0 null:proofs+flag:0x200",
        BAD_M["1,3,2"]: "m_of:1,3,2 nofs+m_of:1,3,2", BAD_M["0,1,1"]: "m_of:0,1,1", BAD_M["2,4,12"]: "m_of:2,4,12",
        BOTH: "both both+count:33554432",
        NOKEY: "index:nokey",
        NEEDS_FS: "nofs nofs+blinding",
    }, {NULL: "null:ws", SHORT: "ws:0", BAD_M["1,3,2"]: "m_of:1,3,2+ws:0"}, {})


def _many_keys(device):
    return _rows(device, {
        "run": "valid count:1 " + AT_PAIRS,
        NULL: "null:v null:proofs null:commitments null:m_of null:keys null:out_masks null:status",
        "0": "count:0 null:proofs+count:0 n_keys:0 null:keys+n_keys:0 null:proofs+n_keys:0 keys:misaligned+n_keys:0",
        PROOF_PAIRS: OVER_PAIRS,
        FLAG: UNKNOWN_BITS % ("proofs", "proofs") + " flag:0x200 flag:0x200+count:0 null:proofs+flag:0x200",
        BAD_M["1,3,2"]: "m_of:1,3,2 nofs+m_of:1,3,2", BAD_M["0,1,1"]: "m_of:0,1,1", BAD_M["2,4,12"]: "m_of:2,4,12",
        NEEDS_FS: "nofs",
    }, {NULL: "null:ws", SHORT: "ws:0", BAD_M["1,3,2"]: "m_of:1,3,2+ws:0", ALIGN: "keys:misaligned"}, {"run": "keys:misaligned"})


def _find(device, tagged):
    """the two rewinding modes: BPP_FIND_AMOUNTS_SEALED is theirs to take"""
    return _rows(device, {
        "run": "valid count:1 n_keys:0 null:keys+n_keys:0 keys:misaligned+n_keys:0 null:hits+max_hits:0 flag:0x200 " + AT_PAIRS,
        NULL: "null:v null:proofs null:commitments null:m_of null:keys null:amounts null:ok null:hits null:n_hits "
              "null:n_hits+count:0 null:n_hits+flag:0x4 null:proofs+n_keys:0 null:proofs+flag:0x200" + (" null:tags" if tagged else ""),
        "0": "count:0 null:proofs+count:0 flag:0x200+count:0",
        PROOF_PAIRS: OVER_PAIRS,
        FLAG: UNKNOWN_BITS % ("proofs", "proofs") + " flag:0x204 flag:0x204+count:0",
        BAD_M["1,3,2"]: "m_of:1,3,2 nofs+m_of:1,3,2", BAD_M["0,1,1"]: "m_of:0,1,1", BAD_M["2,4,12"]: "m_of:2,4,12",
        NEEDS_FS: "nofs",
    }, {NULL: "null:ws", SHORT: "ws:0", BAD_M["1,3,2"]: "m_of:1,3,2+ws:0", ALIGN: "keys:misaligned"}, {"run": "keys:misaligned"})


def _find_outputs(device, ragged):
    """per output: the sealed flag is refused by name ahead of the flags nobody takes; the ragged form leaves its counts to
    the plan"""
    units = "outs_of" if ragged else "m_of"
    common = {
        "run": "valid count:1 n_keys:0 null:keys+n_keys:0 keys:misaligned+n_keys:0 null:hits+max_hits:0 " + AT_PAIRS,
        NULL: "null:v null:proofs null:commitments null:%s null:keys null:amounts null:tags null:ok null:hits null:n_hits "
              "null:n_hits+count:0 null:n_hits+flag:0x4 null:proofs+n_keys:0" % units,
        "0": "count:0 null:proofs+count:0",
        OUTPUT_PAIRS: OVER_PAIRS,
        SEALED: "flag:0x200 flag:0x200+count:0 null:proofs+flag:0x200 flag:0x204 flag:0x204+count:0",
        FLAG: UNKNOWN_BITS % ("proofs", "proofs"),
        VERDICTS_FS: "nofs",
    }
    device_only = {NULL: "null:ws", SHORT: "ws:0", ALIGN: "keys:misaligned"}
    if ragged:
        common["run"] += " outs_of:1,3,2 outs_of:0,1,1 outs_of:2,4,12 outs_of:1,0,2 outs_of:1,129,2"
        common[VERDICTS_FS] += " nofs+outs_of:1,3,2"
        device_only[SHORT] += " outs_of:1,3,2+ws:0"
    else:
        common.update({BAD_M["1,3,2"]: "m_of:1,3,2 nofs+m_of:1,3,2", BAD_M["0,1,1"]: "m_of:0,1,1", BAD_M["2,4,12"]: "m_of:2,4,12"})
        device_only[BAD_M["1,3,2"]] = "m_of:1,3,2+ws:0"
    return _rows(device, common, device_only, {"run": "keys:misaligned"})


TABLE = {
    "bpp_range_recover_masks_mixed_device": _recover(True),
    "bpp_range_recover_masks_mixed": _recover(False),
    "bpp_range_scan_serialized_mixed_device": _one_key(True),
    "bpp_range_scan_serialized_mixed": _one_key(False),
    "bpp_range_scan_serialized_mixed_keys_device": _many_keys(True),
    "bpp_range_scan_serialized_mixed_keys": _many_keys(False),
    "bpp_range_verify_find_serialized_mixed_keys_device": _find(True, False),
    "bpp_range_verify_find_serialized_mixed_keys": _find(False, False),
    "bpp_range_verify_find_tagged_serialized_mixed_keys_device": _find(True, True),
    "bpp_range_verify_find_tagged_serialized_mixed_keys": _find(False, True),
    "bpp_range_verify_find_outputs_serialized_mixed_keys_device": _find_outputs(True, False),
    "bpp_range_verify_find_outputs_serialized_mixed_keys": _find_outputs(False, False),
    "bpp_range_verify_find_outputs_serialized_outs_keys_device": _find_outputs(True, True),
    "bpp_range_verify_find_outputs_serialized_outs_keys": _find_outputs(False, True),
}


def expected(entry, defect):
    """-> TABLE's outcome of (entry, defect)"""
    hit = [out for out, defects in TABLE[entry].items() if defect in defects.split()]
    assert len(hit) == 1, (entry, defect, hit)
    return hit[0]


def test_table_is_a_function_of_entry_and_defect():
    assert len(TABLE) == 14
    for entry, by in TABLE.items():
        seen = [d for defects in by.values() for d in defects.split()]
        assert len(seen) == len(set(seen)), entry
        assert {"valid", "null:v", "count:0", "count:33554432", "count:4294967296"} <= set(seen), entry
        assert ("ws:0" in seen) == entry.endswith("_device"), entry


def test_scan_args_answers_as_the_ladders_did(tmp_path):
    out = subprocess.run([_build("scan_args_host_test", tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = {}
    for line in out.stdout.splitlines():
        entry, defect, res = line.split("\t")
        assert (entry, defect) not in got, (entry, defect)
        got[(entry, defect)] = res
    want = {(entry, d): res for entry, by in TABLE.items() for res, defects in by.items() for d in defects.split()}
    assert len(want) == 601
    assert set(got) == set(want), (sorted(set(got) - set(want))[:10], sorted(set(want) - set(got))[:10])
    wrong = [(k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]
    assert not wrong, wrong[:20]
