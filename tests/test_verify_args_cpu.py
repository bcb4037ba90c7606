"""CPU: the argument checks of the verifier's 19 C entries (csrc/verify_args.hpp: VerifyEntry data, verify_args) answer
every defect as the per-entry ladders of capi.hip did before they became data.

tests/host/verify_args_host_test.cpp (g++, under the sanitizers with BPP_HOST_SANITIZE=1) includes the check header alone
and walks every entry over: each required pointer null, one at a time; count 0, 1, 0x7fffffff/64, one more, 2^32; the flag
bits outside the entry's set; group 0..4; no weight source; n or m of 256; container version 2 on edwards25519; and the
pairs of defects whose winner the ladders' ORDER decides (null with unknown flag, null with count 0, unknown flag with
count 0, count too large with no weight source).  It prints `entry, defect, code, text[, stats]` per row; TABLE below is
what must come out.

Every row of TABLE was derived by reading the ladder of that entry in capi.hip at commit a1134c0 (the last one with
ladders), line by line, not from the new check: "run" is a call that passes the entry's checks and goes on to the
implementation, "0" one the entry answers itself (an empty batch), "-1 text" a refusal with bpp_last_error()'s text, and
"stats zeroed" / "stats kept" whether the entry's own `stats[0] = stats[1] = 0` had run by then.  Things the ladders never
looked at stay "run" here: the group, the engine's n, m <= 255 and the workspace size are refused one layer further in
(LIVE below, what tests/test_gpu_verify_entries.py sees on a live engine; those rows were checked against a build of
a1134c0 on the GPU, as were the "unknown flag", "count:0" and "empty batch" rows of TABLE).  bpp_range_verify_batch_serialized
alone names the flags it does not take BEHIND its other checks: there the text came from the device entry inside the host
form."""

import subprocess

from test_host_arith_cpu import _build

TABLE = {
    "bpp_verifier_run": {
        "run": "valid count:1 count:33554431 n:256 m:256",
        "-1 null argument": "null:v null:points null:scalars null:ok null:ws null:points+count:0",
        "0": "count:0",
        "-1 count too large for one launch": "count:33554432 count:4294967296",
    },
    "bpp_verifier_graph_capture": {
        "run": "valid count:1 count:33554431 n:256 m:256",
        "-1 null argument": "null:v null:points null:scalars null:ok null:ws null:out null:points+count:0",
        "-1 count out of range": "count:0 count:33554432 count:4294967296",
    },
    "bpp_verifier_run_combined": {
        "run": "valid count:1 count:33554431 count:33554432 n:256 m:256",
        "-1 null argument": "null:v null:points null:scalars null:out_partial null:ok null:ws null:points+count:0",
        "-1 empty batch": "count:0",
        "-1 count too large": "count:4294967296",
        "-1 the combined check needs a weight key or a weight buffer": "noweight count:33554432+noweight",
    },
    "bpp_verifier_run_grouped": {
        "run | stats kept":
            "valid count:0 count:1 count:33554431 count:33554432 group:0 group:1 group:2 group:3 group:4 n:256 "
            "m:256 null:points+count:0",
        "-1 null argument | stats kept": "null:v null:points null:scalars null:ok null:ws",
        "-1 count too large | stats kept": "count:4294967296",
        "-1 the grouped check needs a weight key or a weight buffer | stats kept": "noweight count:33554432+noweight",
    },
    "bpp_verifier_grouped_begin": {
        "run":
            "valid count:0 count:1 count:33554431 count:33554432 group:0 group:1 group:2 group:3 group:4 n:256 "
            "m:256 null:points+count:0",
        "-1 null argument": "null:v null:points null:scalars null:ok null:ws",
        "-1 count too large": "count:4294967296",
        "-1 the grouped check needs a weight key or a weight buffer": "noweight count:33554432+noweight",
    },
    "bpp_verifier_grouped_finish": {
        "run | stats kept":
            "valid count:0 count:1 count:33554431 count:33554432 group:0 group:1 group:2 group:3 group:4 n:256 "
            "m:256 null:points+count:0",
        "-1 null argument | stats kept": "null:v null:points null:scalars null:ok null:ws",
        "-1 count too large | stats kept": "count:4294967296",
    },
    "bpp_verifier_derive_challenges": {
        "run": "valid count:1 count:33554431 count:33554432 n:256 m:256",
        "-1 null argument": "null:v null:points null:out_challenges null:points+count:0",
        "0": "count:0",
        "-1 count too large": "count:4294967296",
    },
    "bpp_verifier_run_mixed": {
        "run": "valid count:1 count:33554431 n:256 m:256",
        "-1 null argument": "null:v null:points null:scalars null:m_of null:ok null:ws",
        "0": "count:0 null:points+count:0",
        "-1 count too large for one launch": "count:33554432 count:4294967296",
    },
    "bpp_verifier_derive_challenges_mixed": {
        "run": "valid count:1 count:33554431 n:256 m:256",
        "-1 null argument": "null:v null:points null:m_of null:out_challenges null:ws",
        "0": "count:0 null:points+count:0",
        "-1 count too large for one launch": "count:33554432 count:4294967296",
    },
    "bpp_range_verify_batch_serialized_device": {
        "run": "valid count:1 count:33554431 ed25519:v2 n:256 m:256",
        "-1 null argument": "null:v null:proofs null:commitments null:ok null:ws null:proofs+flag:0x4 null:proofs+count:0",
        "0": "count:0",
        "-1 count too large for one launch": "count:33554432 count:4294967296",
        "-1 unknown flag": "flag:0x4 flag:0x100 flag:0x4+count:0",
    },
    "bpp_range_verify_batch_serialized_grouped_device": {
        "run | stats zeroed": "valid count:1 count:33554431 ed25519:v2 group:0 group:1 group:2 group:3 group:4 n:256 m:256",
        "-1 null argument | stats kept":
            "null:v null:proofs null:commitments null:ok null:ws noweight null:proofs+flag:0x4 "
            "null:proofs+count:0 count:33554432+noweight",
        "0 | stats zeroed": "count:0",
        "-1 count too large for one launch | stats zeroed": "count:33554432 count:4294967296",
        "-1 unknown flag | stats kept": "flag:0x4 flag:0x100 flag:0x4+count:0",
    },
    "bpp_range_verify_batch_serialized_mixed_device": {
        "run": "valid count:1 count:33554431 ed25519:v2 n:256 m:256",
        "-1 null argument": "null:v null:proofs null:commitments null:m_of null:ok null:ws",
        "0": "count:0 null:proofs+count:0",
        "-1 count too large for one launch": "count:33554432 count:4294967296",
        "-1 unknown flag": "flag:0x4 flag:0x100 null:proofs+flag:0x4 flag:0x4+count:0",
    },
    "bpp_verifier_run_grouped_mixed": {
        "run | stats zeroed": "valid count:1 count:33554431 group:0 group:1 group:2 group:3 group:4 n:256 m:256",
        "-1 null argument | stats kept": "null:v",
        "-1 null argument | stats zeroed": "null:points null:scalars null:m_of null:ok null:ws",
        "0 | stats zeroed": "count:0 null:points+count:0",
        "-1 count too large for one launch | stats zeroed": "count:33554432 count:4294967296",
        "-1 the grouped check needs a weight key or a weight buffer | stats zeroed": "noweight count:33554432+noweight",
    },
    "bpp_range_verify_batch_serialized_grouped_mixed_device": {
        "run | stats zeroed": "valid count:1 count:33554431 ed25519:v2 group:0 group:1 group:2 group:3 group:4 n:256 m:256",
        "-1 null argument | stats kept": "null:v",
        "-1 null argument | stats zeroed": "null:proofs null:commitments null:m_of null:ok null:ws noweight count:33554432+noweight",
        "0 | stats zeroed": "count:0 null:proofs+count:0",
        "-1 count too large for one launch | stats zeroed": "count:33554432 count:4294967296",
        "-1 unknown flag | stats kept": "flag:0x4 flag:0x100 null:proofs+flag:0x4 flag:0x4+count:0",
    },
    "bpp_range_verify_batch": {
        "run": "valid count:1 count:33554431 count:33554432 n:256 m:256",
        "-1 null argument": "null:v null:points null:scalars null:ok null:points+count:0",
        "0": "count:0",
        "-1 count too large": "count:4294967296",
    },
    "bpp_range_verify_batch_mixed": {
        "run": "valid count:1 count:33554431 count:33554432 n:256 m:256",
        "-1 null argument": "null:v null:points null:scalars null:m_of null:ok",
        "0": "count:0 null:points+count:0",
        "-1 count too large": "count:4294967296",
    },
    "bpp_range_verify_batch_compressed": {
        "run": "valid count:1 count:33554431 count:33554432 n:256 m:256",
        "-1 null argument": "null:v null:records null:scalars null:ok null:records+count:0",
        "0": "count:0",
        "-1 count too large": "count:4294967296",
    },
    "bpp_range_verify_batch_serialized": {
        "run": "valid count:1 count:33554431 count:33554432",
        "-1 null argument": "null:v null:proofs null:commitments null:ok null:proofs+flag:0x4 null:proofs+count:0",
        "0": "count:0 flag:0x4+count:0",
        "-1 count too large": "count:4294967296",
        "-1 unknown flag": "flag:0x4 flag:0x100",
        "-1 n*m must be a power of two (n, m <= 255)": "ed25519:v2 n:256 m:256",
    },
    "bpp_range_verify_batch_serialized_mixed": {
        "run": "valid count:1 count:33554431 count:33554432 n:256 m:256",
        "-1 null argument": "null:v null:proofs null:commitments null:m_of null:ok",
        "0": "count:0 null:proofs+count:0",
        "-1 count too large": "count:4294967296",
        "-1 unknown flag": "flag:0x4 flag:0x100 null:proofs+flag:0x4 flag:0x4+count:0",
        "-1 container version 2 (uncompressed points) is not offered for this curve": "ed25519:v2",
    },
}

# What a LIVE engine answers where TABLE says "run" and the implementation behind the entry refuses: read from
# impl_verify.hpp at a1134c0 (check_group ahead of the layout in the grouped forms; behind the decoder and the plan in the
# serialized and mixed ones; "workspace too small" behind the layout everywhere), for a batch of 3 proofs.
GROUP_TEXT = "-1 group must be a power of two, at least 2"
SHORT_TEXT = "-1 workspace too small"
LIVE = {
    ("bpp_verifier_run_grouped", "group:3"): GROUP_TEXT + " | stats kept",
    ("bpp_verifier_grouped_begin", "group:3"): GROUP_TEXT,
    ("bpp_verifier_grouped_finish", "group:3"): GROUP_TEXT + " | stats kept",
    ("bpp_range_verify_batch_serialized_grouped_device", "group:3"): GROUP_TEXT + " | stats zeroed",
    ("bpp_verifier_run_grouped_mixed", "group:3"): GROUP_TEXT + " | stats zeroed",
    ("bpp_range_verify_batch_serialized_grouped_mixed_device", "group:3"): GROUP_TEXT + " | stats zeroed",
    ("bpp_verifier_run", "ws:short"): SHORT_TEXT,
    ("bpp_verifier_graph_capture", "ws:short"): SHORT_TEXT,
    ("bpp_verifier_run_combined", "ws:short"): SHORT_TEXT,
    ("bpp_verifier_run_grouped", "ws:short"): SHORT_TEXT + " | stats kept",
    ("bpp_verifier_grouped_begin", "ws:short"): SHORT_TEXT,
    ("bpp_verifier_grouped_finish", "ws:short"): SHORT_TEXT + " | stats kept",
    ("bpp_verifier_run_mixed", "ws:short"): SHORT_TEXT,
    ("bpp_verifier_derive_challenges_mixed", "ws:short"): SHORT_TEXT,
    ("bpp_range_verify_batch_serialized_device", "ws:short"): SHORT_TEXT,
    ("bpp_range_verify_batch_serialized_grouped_device", "ws:short"): SHORT_TEXT + " | stats zeroed",
    ("bpp_range_verify_batch_serialized_mixed_device", "ws:short"): SHORT_TEXT,
    ("bpp_verifier_run_grouped_mixed", "ws:short"): SHORT_TEXT + " | stats zeroed",
    ("bpp_range_verify_batch_serialized_grouped_mixed_device", "ws:short"): SHORT_TEXT + " | stats zeroed",
    # an empty batch that the grouped entries pass on: both halves answer it, the second behind its own stats write
    ("bpp_verifier_run_grouped", "count:0"): "0 | stats zeroed",
    ("bpp_verifier_grouped_begin", "count:0"): "0",
    ("bpp_verifier_grouped_finish", "count:0"): "0 | stats zeroed",
}


def expected(entry, defect):
    """-> TABLE's outcome of (entry, defect); where that is "run", LIVE's (None: the call runs to its end)"""
    hit = [out for out, defects in TABLE[entry].items() if defect in defects.split()]
    assert len(hit) <= 1, (entry, defect, hit)
    out = hit[0] if hit else "run"
    if out.split(" | ")[0] == "run":
        return LIVE.get((entry, defect))
    return out


def test_table_is_a_function_of_entry_and_defect():
    assert len(TABLE) == 19
    for entry, by in TABLE.items():
        seen = [d for defects in by.values() for d in defects.split()]
        assert len(seen) == len(set(seen)), entry
        assert {"valid", "null:v", "count:0", "count:4294967296", "n:256", "m:256"} <= set(seen), entry


def test_verify_args_answers_as_the_ladders_did(tmp_path):
    out = subprocess.run([_build("verify_args_host_test", tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = {}
    for line in out.stdout.splitlines():
        entry, defect, res = line.split("\t")
        assert (entry, defect) not in got, (entry, defect)
        got[(entry, defect)] = res
    want = {(entry, d): res for entry, by in TABLE.items() for res, defects in by.items() for d in defects.split()}
    assert len(want) == 339
    assert set(got) == set(want), (sorted(set(got) - set(want))[:10], sorted(set(want) - set(got))[:10])
    wrong = [(k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]
    assert not wrong, wrong[:20]
