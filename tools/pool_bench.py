#!/usr/bin/env python3
"""What the verifier pool costs on ONE device: a block of serialized range proofs of mixed aggregation sizes handed over as
host bytes, verified by

  i    bpp_range_verify_batch_serialized_mixed on a plain verifier (allocates its device buffers per call)
  ii   bpp_pool_verify_serialized_mixed on a pool of one shard (buffers kept across calls, one worker thread)
  iii  the same on a pool of two shards, both on device 0 (two passes sharing one device: informative only)

the three ALTERNATED repetition by repetition and timed by the wall clock: every call is synchronous and takes host
pointers, so the wall clock is what a caller sees.  The block: BLS12-381, n = 64, capacity m = 16; 8 192 distinct proofs made
under the transcript by the batched prover, m_i distributed 4096 / 2048 / 1024 / 512 / 512 over m_i = 1 / 2 / 4 / 8 / 16,
shuffled, a handful with a flipped s'.  The status vectors of the three legs are compared after every repetition.  Scaling
over several real devices is not something one device can show.  Prints one JSON object.
usage: python tools/pool_bench.py [--reps 20] [--warmup 3] [--window 13] [--scale 1.0] [--out profiles/pool_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N = 64
CAP = 16
MIX = {1: 4096, 2: 2048, 4: 1024, 8: 512, 16: 512}


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "stdev_ms": statistics.stdev(ms) if len(ms) > 1 else 0.0, "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=int, default=13)
    ap.add_argument("--tamper", type=int, default=8, help="proofs with a flipped s'")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="scales the proof counts (rehearsals)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pool_bench needs a GPU: nothing here is measured on the CPU")
    import bulletproofsplus_amd as B
    rng = np.random.default_rng(args.seed)
    a = B.Arith("bls12_381")
    pk = B.PublicKey.new(a, N * CAP)
    build_s = {}
    t0 = time.perf_counter()
    plain = B.BatchVerifier(pk, N, CAP, window_bits=args.window)
    build_s["plain"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    pool1 = B.VerifierPool(pk, N, CAP, window_bits=args.window, devices=(0,))
    build_s["pool_1"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    pool2 = B.VerifierPool(pk, N, CAP, window_bits=args.window, devices=(0, 0))
    build_s["pool_2_concurrent"] = time.perf_counter() - t0

    # the block in caller order: shuffled sizes, every proof distinct, proved as bytes by the capacity engine
    ms = [m for m, cnt in MIX.items() for _ in range(max(1, int(cnt * args.scale)))]
    ms = [ms[p] for p in rng.permutation(len(ms))]
    count = len(ms)
    vals = [rng.integers(0, 1 << 31, size=m, dtype=np.uint64).tolist() for m in ms]    # RangeProver::commit takes v as i32
    gams = [[int(g) for g in rng.integers(1, 1 << 62, size=m, dtype=np.uint64)] for m in ms]
    raw, cm, ms_out = plain.prove_serialized_mixed(vals, gams, transcript=True)
    assert ms_out.tolist() == ms
    raw = np.frombuffer(raw, dtype=np.uint8).copy()
    cm = np.frombuffer(cm, dtype=np.uint8).copy()
    ends = np.cumsum([B.proof_bytes(a, N, m) for m in ms])
    victims = sorted(int(t) for t in rng.choice(count, size=min(args.tamper, count), replace=False))
    for t in victims:
        raw[ends[t] - 64] ^= 1    # the low byte of s'
    want = [1 if t in set(victims) else 0 for t in range(count)]

    legs = {
        "i_plain_host_call": lambda: plain.verify_serialized_mixed(raw, cm, ms, transcript=True),
        "ii_pool_one_shard": lambda: pool1.verify_serialized_mixed(raw, cm, ms, transcript=True),
        "iii_pool_two_shards_one_device": lambda: pool2.verify_serialized_mixed(raw, cm, ms, transcript=True),
    }
    identical = True
    for _ in range(args.warmup):
        for f in legs.values():
            identical &= f().tolist() == want
    times = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, f in legs.items():
            t0 = time.perf_counter()
            ok = f()
            times[k].append((time.perf_counter() - t0) * 1e3)
            identical &= ok.tolist() == want
    res = {"device": torch.cuda.get_device_name(0), "curve": "bls12_381", "n": N, "capacity_m": CAP, "window_bits": args.window,
           "count": count, "mix": {str(m): ms.count(m) for m in MIX}, "bytes": {"proofs": int(len(raw)), "commitments": int(len(cm))},
           "tampered": len(victims), "clock": "wall, host call to host return", "table_build_s": build_s,
           "cuts_two_shards": pool2.cuts(ms).tolist(), "legs": {k: stats(v) for k, v in times.items()},
           "statuses_identical_and_as_expected": bool(identical)}
    med = {k: statistics.median(v) for k, v in times.items()}
    res["ratio_ii_over_i"] = med["ii_pool_one_shard"] / med["i_plain_host_call"]
    res["ratio_iii_over_i"] = med["iii_pool_two_shards_one_device"] / med["i_plain_host_call"]
    res["verifies_per_s"] = {k: count / (m / 1e3) for k, m in med.items()}
    res["multi_device_scaling"] = "unmeasured"
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    pool2.close()
    pool1.close()
    plain.close()


if __name__ == "__main__":
    main()
