#!/usr/bin/env python3
"""Times the ragged calls (any number of outputs per proof) against the padded ones on one MI355X.

BLS12-381, the (64, 16) engine, a block of 2^14 containers whose output counts cycle through 2, 3, 5, 6, 3, 2, under the
transcript.  The legs of each pair alternate in one process, device events around calls that end in a synchronise:
  verify : bpp_range_verify_batch_serialized_outs_device against bpp_range_verify_batch_serialized_mixed_device on the same
           proofs with the identity encodings appended
  find   : the same pair for the find-outputs call under 64 keys, dummy sealed and tag entries on the padded side
  prove  : bpp_range_prove_batch_serialized_outs_device against the mixed prove call on zero-padded inputs
No ratio is expected in advance; the saving is bounded by the counts (21 of 110 commitment decodes and pair columns).

--parent LIB: also runs the tools/mixed_bench.py serialized leg (outs_of = NULL) on this build and on the library at LIB
(a build of the parent commit), alternated, each twice, in child processes, and reports the difference of the medians
beside the spread of the two parent runs.

usage: python tools/outs_bench.py [--count 16384] [--reps 10] [--warmup 2] [--window 16] [--keys 64] [--parent LIB [--parent-only]]
                                  [--out profiles/outs_bench.json]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N, CAP = 64, 16
CYCLE = (2, 3, 5, 6, 3, 2)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def alternated(torch, legs, reps, warmup):
    """legs: {name: fn}; every round runs each leg once, in turn -> {name: [ms]}"""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1))
    return out


def pair(res):
    a, b = stats(res["outs"]), stats(res["padded"])
    return {"outs": a, "padded": b, "ratio_outs_over_padded": a["median_ms"] / b["median_ms"]}


def parent_leg(args):
    """the serialized mixed leg of tools/mixed_bench.py on this build and on the parent's, alternated, each twice"""
    runs = {"this": [], "parent": []}
    for which in ("this", "parent", "this", "parent"):
        env = dict(os.environ)
        if which == "parent":
            env["BPP_AMD_LIB"] = os.path.abspath(args.parent)
        else:
            env.pop("BPP_AMD_LIB", None)
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "leg.json")
            subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mixed_bench.py"), "--serialized", "--mixed-only",
                            "--reps", str(args.reps), "--window", str(args.window), "--out", out], check=True, env=env,
                           stdout=subprocess.DEVNULL)
            runs[which].append(json.load(open(out)))

    def median(r):   # the leg's own record of the mixed call
        for key in ("mixed", "serialized_mixed", "leg_a"):
            if key in r and isinstance(r[key], dict) and "median_ms" in r[key]:
                return r[key]["median_ms"]
        raise KeyError("no median of the mixed leg in %s" % sorted(r))

    this, parent = [median(r) for r in runs["this"]], [median(r) for r in runs["parent"]]
    return {"this_median_ms": this, "parent_median_ms": parent,
            "difference_ms": statistics.mean(this) - statistics.mean(parent), "parent_spread_ms": abs(parent[0] - parent[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1 << 14)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--keys", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--parent-only", action="store_true", help="only the comparison with --parent; merged into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outs_bench.json"))
    args = ap.parse_args()
    if args.parent_only:
        res = json.load(open(args.out)) if os.path.exists(args.out) else {}
        res["serialized_mixed_against_parent"] = parent_leg(args)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["serialized_mixed_against_parent"]))
        return
    import torch
    import bulletproofsplus_amd as B
    dev = torch.device("cuda:0")
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    rng = np.random.default_rng(args.seed)
    a = B.Arith("bls12_381")
    bv = B.BatchVerifier(B.PublicKey.new(a, N * CAP), N, CAP, window_bits=args.window)
    outs = np.array([CYCLE[i % len(CYCLE)] for i in range(args.count)], dtype=np.uint32)
    shapes = B.outs_shapes(outs, CAP)
    n_out, n_pad = int(outs.sum()), int(shapes.sum())
    pb = B.compressed_bytes(a)
    nbytes = sum(B.proof_bytes(a, N, int(m)) for m in shapes)

    def dev_of(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)

    # the witnesses: real outputs, and the same zero-padded to the shapes; masks from the recipients' keys (the find leg)
    keys = [hashlib.sha256(b"outs_bench key %d" % q).digest() for q in range(args.keys)]
    owner = rng.integers(0, args.keys + 1, size=n_out)   # one in keys + 1 belongs to nobody who scans
    foreign = hashlib.sha256(b"outs_bench foreign").digest()
    amounts = rng.integers(0, 1 << 31, size=n_out, dtype=np.uint64)
    masks, sealed, tags = bv.make_outputs([keys[q] if q < args.keys else foreign for q in owner], amounts, outs, index_base=7)
    first = np.concatenate([[0], np.cumsum(outs)]).astype(int)
    pfirst = np.concatenate([[0], np.cumsum(shapes)]).astype(int)
    pv = np.zeros(n_pad, dtype=np.uint64)
    pg = np.zeros((n_pad, 4), dtype=np.uint64)
    pse = np.zeros(n_pad, dtype=np.uint64)
    ptg = np.zeros(n_pad, dtype=np.uint8)
    for i in range(args.count):
        o = int(outs[i])
        pv[pfirst[i]:pfirst[i] + o] = amounts[first[i]:first[i] + o]
        pg[pfirst[i]:pfirst[i] + o] = masks[first[i]:first[i] + o]
        pse[pfirst[i]:pfirst[i] + o] = sealed[first[i]:first[i] + o]
        ptg[pfirst[i]:pfirst[i] + o] = tags[first[i]:first[i] + o]
    d_v, d_g, d_pv, d_pg = dev_of(amounts), dev_of(masks), dev_of(pv), dev_of(pg)
    d_raw = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    d_raw2 = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    d_cm = torch.zeros(n_out * pb, dtype=torch.uint8, device=dev)
    d_pcm = torch.zeros(n_pad * pb, dtype=torch.uint8, device=dev)
    sender = hashlib.sha256(b"outs_bench sender").digest()
    kw = dict(transcript=True, blind_key=sender, index_base=7)
    wp, wpp = bv.prover_serialized_outs_workspace_bytes(outs), bv.prover_mixed_workspace_bytes(shapes, serialized=True)
    d_wp = torch.empty(max(wp, wpp), dtype=torch.uint8, device=dev)

    def prove_outs():
        bv.prove_serialized_outputs_device(d_v.data_ptr(), d_g.data_ptr(), outs, d_raw.data_ptr(), d_cm.data_ptr(), d_wp.data_ptr(),
                                           wp, stream(), **kw)
        torch.cuda.synchronize()

    def prove_padded():
        bv.prove_serialized_mixed_device(d_pv.data_ptr(), d_pg.data_ptr(), shapes, d_raw2.data_ptr(), d_pcm.data_ptr(),
                                         d_wp.data_ptr(), wpp, stream(), **kw)
        torch.cuda.synchronize()

    res = {"block": {"count": args.count, "outs_cycle": list(CYCLE), "outputs": n_out, "padded_outputs": n_pad,
                     "padded_commitment_bytes": (n_pad - n_out) * pb, "keys": args.keys, "window_bits": args.window}}
    res["prove"] = pair(alternated(torch, {"outs": prove_outs, "padded": prove_padded}, args.reps, args.warmup))
    assert torch.equal(d_raw, d_raw2), "the ragged prover's containers are the padded prover's"
    d_ok = torch.zeros(args.count, dtype=torch.int32, device=dev)
    d_ok2 = torch.zeros(args.count, dtype=torch.int32, device=dev)
    wv, wvp = bv.serialized_outs_workspace_bytes(outs), bv.serialized_mixed_workspace_bytes(shapes)
    d_wv = torch.empty(max(wv, wvp), dtype=torch.uint8, device=dev)

    def verify_outs():
        bv.verify_serialized_outputs_device(d_raw.data_ptr(), d_cm.data_ptr(), outs, d_ok.data_ptr(), d_wv.data_ptr(), wv, stream(),
                                            transcript=True)
        torch.cuda.synchronize()

    def verify_padded():
        bv.verify_serialized_mixed_device(d_raw.data_ptr(), d_pcm.data_ptr(), shapes, d_ok2.data_ptr(), d_wv.data_ptr(), wvp,
                                          stream(), transcript=True)
        torch.cuda.synchronize()

    res["verify"] = pair(alternated(torch, {"outs": verify_outs, "padded": verify_padded}, args.reps, args.warmup))
    assert torch.equal(d_ok, d_ok2) and int(d_ok.sum()) == 0, "both legs accept the block"
    d_keys = dev_of(np.frombuffer(b"".join(keys), dtype=np.uint8))
    d_se, d_tg, d_pse, d_ptg = dev_of(sealed), dev_of(tags), dev_of(pse), dev_of(ptg)
    cap_hits = n_out
    d_hits = torch.zeros(cap_hits * 12, dtype=torch.int32, device=dev)
    d_n = torch.zeros(4, dtype=torch.int32, device=dev)
    wf, wfp = bv.verify_find_outputs_outs_workspace_bytes(outs, args.keys), bv.verify_find_outputs_workspace_bytes(shapes, args.keys)
    d_wf = torch.empty(max(wf, wfp), dtype=torch.uint8, device=dev)

    def find_outs():
        bv.verify_find_outputs_serialized_outs_keys_device(d_raw.data_ptr(), d_cm.data_ptr(), outs, d_keys.data_ptr(), args.keys,
                                                           d_se.data_ptr(), d_tg.data_ptr(), d_ok.data_ptr(), d_hits.data_ptr(),
                                                           cap_hits, d_n.data_ptr(), d_wf.data_ptr(), wf, stream(), index_base=7,
                                                           d_n_candidates=d_n.data_ptr() + 4)
        torch.cuda.synchronize()

    def find_padded():
        bv.verify_find_outputs_serialized_mixed_keys_device(d_raw.data_ptr(), d_pcm.data_ptr(), shapes, d_keys.data_ptr(), args.keys,
                                                            d_pse.data_ptr(), d_ptg.data_ptr(), d_ok2.data_ptr(), d_hits.data_ptr(),
                                                            cap_hits, d_n.data_ptr() + 8, d_wf.data_ptr(), wfp, stream(),
                                                            index_base=7, d_n_candidates=d_n.data_ptr() + 12)
        torch.cuda.synchronize()

    res["find"] = pair(alternated(torch, {"outs": find_outs, "padded": find_padded}, args.reps, args.warmup))
    n = d_n.cpu().tolist()
    owned = int((owner < args.keys).sum())
    assert n[0] == n[2] == owned, "both legs find every owned output: %s, %d owned" % (n, owned)
    res["find"]["hits"], res["find"]["candidates_outs"], res["find"]["candidates_padded"] = n[0], n[1], n[3]
    bv.close()
    if args.parent:
        res["serialized_mixed_against_parent"] = parent_leg(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
