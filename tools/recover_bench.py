#!/usr/bin/env python3
"""What a scan costs beside a verification of the same block.  One process, BLS12-381, a (64, 16) engine; every
GPU step runs under an alarm of its own (a SLOW step ends the run there, with what was measured so far written out).  The
alarm is raised only when the interpreter has control again, so run the whole tool under `timeout -k 10 <seconds>` as well.

  scan     bpp_range_scan_serialized_mixed_device and bpp_range_verify_batch_serialized_mixed_device on the same block of
           containers, alternated repetition by repetition: medians, ranges, the ratio scan / verify.  Two blocks, both made
           by the device prover under the transcript with a blind key: `mixed`, the 8 192-proof block of DESIGN 4f (4 096 x
           m = 1, 2 048 x 2, 1 024 x 4, 512 x 8, 512 x 16, shuffled), and `wallet`, 2^16 containers with m = 1 and a
           candidate amount each.
  recover  bpp_range_recover_masks_mixed_device alone (triples and challenge blocks resident) at 2^12 and 2^16 single-output
           proofs: masks per second.
  keys     (--keys K[,K..]; --legs k) bpp_range_scan_serialized_mixed_keys_device under K keys against K calls of
           bpp_range_scan_serialized_mixed_device, one per key, on the `wallet` block: same process, alternated repetition
           by repetition; both medians, their ratio with the spread of the per-repetition ratios.  --side many|single runs
           one side alone (the run to put under rocprofv3 --kernel-trace --stats); --kernel-stats SIDE=CSV[,SIDE=CSV] folds
           such runs' k_kernel_stats.csv into an existing --out file as the per-kernel split (no GPU needed).
  find     (--find --keys K[,K..]) bpp_range_verify_find_serialized_mixed_keys_device with sealed amounts plus the copy of
           d_ok, d_n_hits and the hit records to the host, against what a caller does today -- verify_serialized_mixed_device,
           scan_serialized_mixed_keys_device, the copy of the verdicts and of the dense pair matrix -- on the `wallet` block,
           alternated repetition by repetition.  The verdicts and the hit list are checked: a wrong one ends the
           run with an error and the file says complete: false.  --side fused|today
           runs one side alone; --kernel-stats fused=CSV,today=CSV folds their per-kernel split in.  The leg's result is
           merged into an existing --out file under "find"; the other legs' results there stay.
  tags     (--find --tags --keys K[,K..]) bpp_range_verify_find_tagged_serialized_mixed_keys_device against the untagged find
           call ON THE SAME BUILD and against the call with no keys (the front and the pass alone), each with its copies to
           the host, on the `wallet` block with the owner's view tags, alternated repetition by repetition:
           medians, spreads, tagged / untagged with the per-repetition spread, and n_candidates / pairs.  Verdicts, hits and
           the candidate count (against hashlib) are checked.  Merged into --out under "find_tags".
  outputs  (--find --outputs --keys K[,K..], default 16,64,256) bpp_range_verify_find_outputs_serialized_mixed_keys_device on
           2^14 containers of m = 4 (2^16 outputs with derived masks, the owner's tags) against the tagged find call on the
           `wallet` block of 2^16 single outputs, each also with n_keys = 0, alternated repetition by repetition (DESIGN.md
           4m): medians, each call's key-dependent part (the call minus its own n_keys = 0 run) and the spread.  Hits and the
           candidate count (against hashlib, every pair) are checked.  Merged into --out under "find_outputs".
usage: timeout -k 10 1100 python tools/recover_bench.py [--reps 20] [--warmup 3] [--window 13] [--scale 1.0] [--legs sr]
       [--blocks mixed,wallet] [--keys 1,4,16,64] [--find] [--tags] [--outputs] [--side both]
       [--out profiles/recover_bench.json]"""
import argparse
import csv
import hashlib
import json
import os
import signal
import statistics
import struct
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

N, CAP = 64, 16
KEY = bytes(range(1, 33))
BASE = 1 << 40


class StepTimeout(Exception):
    pass


def step(seconds, fn):
    """fn() under an alarm of its own"""
    def on_alarm(signum, frame):
        raise StepTimeout()
    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(int(seconds))
    try:
        return fn()
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "stdev_ms": statistics.stdev(ms) if len(ms) > 1 else 0.0, "reps": len(ms)}


def alternate(torch, fns, reps, warmup):
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            out[i].append(e0.elapsed_time(e1))
    return out


def block_shapes(name, scale):
    rng = np.random.default_rng(7)
    if name == "mixed":
        counts = {1: 4096, 2: 2048, 4: 1024, 8: 512, 16: 512}
        ms = np.concatenate([np.full(max(1, int(c * scale)), m) for m, c in counts.items()])
        return ms[rng.permutation(len(ms))].astype(np.uint32)
    return np.ones(max(1, int((1 << 16) * scale)), dtype=np.uint32)


def make_block(torch, B, a, bv, ms):
    """the block as containers, by the device prover -> (d_proofs, d_commitments, d_amounts)"""
    rng = np.random.default_rng(11)
    nval = int(ms.sum())
    vals = rng.integers(0, 1 << 31, size=nval, dtype=np.uint64)
    gams = np.zeros((nval, 4), dtype=np.uint64)
    gams[:, :3] = rng.integers(0, 1 << 62, size=(nval, 3), dtype=np.uint64)
    dev = torch.device("cuda:0")
    d_v = torch.from_numpy(vals.view(np.int64)).to(dev)
    d_g = torch.from_numpy(gams.view(np.int64)).to(dev)
    pb = B.compressed_bytes(a)
    nbytes = sum(int((ms == m).sum()) * B.proof_bytes(a, N, int(m)) for m in np.unique(ms))
    d_p = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    d_c = torch.zeros(nval * pb, dtype=torch.uint8, device=dev)
    wsb = bv.prover_mixed_workspace_bytes(ms, serialized=True)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    bv.prove_serialized_mixed_device(d_v.data_ptr(), d_g.data_ptr(), ms, d_p.data_ptr(), d_c.data_ptr(), d_ws.data_ptr(), wsb,
                                     torch.cuda.current_stream().cuda_stream, transcript=True, blind_key=KEY, index_base=BASE)
    torch.cuda.synchronize()
    del d_ws
    first = np.concatenate([[0], np.cumsum(ms)[:-1]]).astype(int)   # the candidate amount of a proof: its first value
    d_a = torch.from_numpy(vals[first].view(np.int64)).to(dev)
    return d_p, d_c, d_a


def scan_leg(torch, B, a, bv, name, args, out):
    ms = block_shapes(name, args.scale)
    count = len(ms)
    d_p, d_c, d_a = step(600, lambda: make_block(torch, B, a, bv, ms))
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    vsb, ssb = bv.serialized_mixed_workspace_bytes(ms), bv.recover_workspace_bytes(ms, serialized=True)
    d_vws = torch.empty(vsb, dtype=torch.uint8, device=dev)
    d_sws = torch.empty(ssb, dtype=torch.uint8, device=dev)
    d_ok = torch.full((count,), 7, dtype=torch.int32, device=dev)
    d_st = torch.full((count,), 7, dtype=torch.int32, device=dev)
    d_m = torch.zeros((count, 4), dtype=torch.int64, device=dev)

    def verify():
        bv.verify_serialized_mixed_device(d_p.data_ptr(), d_c.data_ptr(), ms, d_ok.data_ptr(), d_vws.data_ptr(), vsb, st,
                                          transcript=True)

    def scan():
        bv.scan_serialized_mixed_device(d_p.data_ptr(), d_c.data_ptr(), ms, d_m.data_ptr(), d_st.data_ptr(), d_sws.data_ptr(),
                                        ssb, st, transcript=True, blind_key=KEY, index_base=BASE, d_amounts=d_a.data_ptr())

    t_scan, t_ver = step(600, lambda: alternate(torch, [scan, verify], args.reps, args.warmup))
    status = d_st.cpu().numpy()
    want = np.where(ms == 1, 0, 3)
    res = {"count": count, "classes": {int(m): int((ms == m).sum()) for m in np.unique(ms)}, "scan": stats(t_scan),
           "verify": stats(t_ver), "ratio_scan_over_verify": statistics.median(t_scan) / statistics.median(t_ver),
           "scans_per_s": count / (statistics.median(t_scan) * 1e-3), "verdicts_all_ok": bool((d_ok.cpu().numpy() == 0).all()),
           "status_as_expected": bool((status == want).all()), "scan_workspace_bytes": ssb, "verify_workspace_bytes": vsb}
    out["scan"][name] = res
    print(name, json.dumps(res), flush=True)


def recover_leg(torch, B, a, bv, log2n, args, out):
    """the recover-only wire call: triples and challenges of 2^log2n single-output proofs, resident"""
    count = max(1, int((1 << log2n) * args.scale))
    ms = np.ones(count, dtype=np.uint32)
    rng = np.random.default_rng(13)
    dev = torch.device("cuda:0")
    k = (N).bit_length() - 1
    sc = np.zeros((count, 3, 4), dtype=np.uint64)
    sc[:, :, :3] = rng.integers(0, 1 << 62, size=(count, 3, 3), dtype=np.uint64)
    ch = np.zeros((count, 3 + k, 4), dtype=np.uint64)
    ch[:, :, :3] = rng.integers(1, 1 << 62, size=(count, 3 + k, 3), dtype=np.uint64)
    d_sc = torch.from_numpy(sc.view(np.int64)).to(dev)
    d_ch = torch.from_numpy(ch.view(np.int64)).to(dev)
    d_m = torch.zeros((count, 4), dtype=torch.int64, device=dev)
    wsb = bv.recover_workspace_bytes(ms)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def run():
        bv.recover_masks_device(d_sc.data_ptr(), ms, d_m.data_ptr(), d_ws.data_ptr(), wsb, st, d_challenges=d_ch.data_ptr(),
                                blind_key=KEY, index_base=BASE)

    (t,) = step(300, lambda: alternate(torch, [run], args.reps, args.warmup))
    res = dict(stats(t), count=count, masks_per_s=count / (statistics.median(t) * 1e-3))
    out["recover"]["2^%d" % log2n] = res
    print("recover 2^%d" % log2n, json.dumps(res), flush=True)


def keys_leg(torch, B, a, bv, ks, args, out):
    """the K-key scan against K single-key scans of the wallet block; key 0 made the block, the others own nothing"""
    ms = block_shapes("wallet", args.scale)
    count = len(ms)
    d_p, d_c, d_a = step(600, lambda: make_block(torch, B, a, bv, ms))
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    ssb = bv.recover_workspace_bytes(ms, serialized=True)
    d_sws = torch.empty(ssb, dtype=torch.uint8, device=dev)
    d_st1 = torch.full((count,), 7, dtype=torch.int32, device=dev)
    d_m1 = torch.zeros((count, 4), dtype=torch.int64, device=dev)
    out["keys"] = {"block": "wallet", "count": count, "side": args.side, "by_keys": {}}
    for K in ks:
        keys = [KEY] + [hashlib.sha256(b"recover_bench key %d" % j).digest() for j in range(1, K)]
        d_keys = torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).to(dev)
        d_am = d_a.repeat(K)
        ksb = bv.scan_keys_workspace_bytes(ms, K)
        d_kws = torch.empty(ksb, dtype=torch.uint8, device=dev)
        d_stK = torch.full((K, count), 7, dtype=torch.int32, device=dev)
        d_mK = torch.zeros((K, count, 4), dtype=torch.int64, device=dev)

        def many():
            bv.scan_serialized_mixed_keys_device(d_p.data_ptr(), d_c.data_ptr(), ms, d_keys.data_ptr(), K, d_mK.data_ptr(),
                                                 d_stK.data_ptr(), d_kws.data_ptr(), ksb, st, index_base=BASE,
                                                 d_amounts=d_am.data_ptr())

        def single():
            for key in keys:
                bv.scan_serialized_mixed_device(d_p.data_ptr(), d_c.data_ptr(), ms, d_m1.data_ptr(), d_st1.data_ptr(),
                                                d_sws.data_ptr(), ssb, st, transcript=True, blind_key=key, index_base=BASE,
                                                d_amounts=d_a.data_ptr())

        fns = {"both": [many, single], "many": [many], "single": [single]}[args.side]
        ts = step(900, lambda: alternate(torch, fns, args.reps, args.warmup))
        res = {"pairs": K * count, "keys_workspace_bytes": ksb, "single_workspace_bytes": ssb}
        if args.side in ("both", "many"):
            status = d_stK.cpu().numpy()
            res["many"] = stats(ts[0])
            res["pairs_per_s"] = K * count / (statistics.median(ts[0]) * 1e-3)
            res["status_as_expected"] = bool((status[0] == 0).all() and (status[1:] == 1).all())
        if args.side in ("both", "single"):
            res["single_x_K"] = stats(ts[-1])
        if args.side == "both":
            per_rep = [m / s for m, s in zip(ts[0], ts[1])]
            res["ratio_many_over_single"] = statistics.median(ts[0]) / statistics.median(ts[1])
            res["ratio_per_rep"] = {"median": statistics.median(per_rep), "min": min(per_rep), "max": max(per_rep)}
        out["keys"]["by_keys"][str(K)] = res
        print("keys %d" % K, json.dumps(res), flush=True)
        del d_keys, d_am, d_kws, d_stK, d_mK


def find_leg(torch, B, a, bv, ks, args, out):
    """the fused verify-and-find call against verify + K-key scan + the copy of the pair matrix; key 0 made the block"""
    ms = block_shapes("wallet", args.scale)
    count = len(ms)
    d_p, d_c, d_a = step(600, lambda: make_block(torch, B, a, bv, ms))
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    d_sealed = torch.zeros_like(d_a)
    bv.seal_amounts_device(KEY, d_a.data_ptr(), count, d_sealed.data_ptr(), st, index_base=BASE)
    vsb = bv.serialized_mixed_workspace_bytes(ms)
    d_vws = torch.empty(vsb, dtype=torch.uint8, device=dev)
    d_ok_f = torch.full((count,), 7, dtype=torch.int32, device=dev)
    d_ok_t = torch.full((count,), 7, dtype=torch.int32, device=dev)
    h_ok_f = torch.empty((count,), dtype=torch.int32, pin_memory=True)
    h_ok_t = torch.empty((count,), dtype=torch.int32, pin_memory=True)
    max_hits = count   # room for every output of one key
    d_hits = torch.zeros((max_hits, 12), dtype=torch.int32, device=dev)
    h_hits = torch.empty((max_hits, 12), dtype=torch.int32, pin_memory=True)
    d_n = torch.zeros((1,), dtype=torch.int32, device=dev)
    out["find"] = {"block": "wallet", "count": count, "side": args.side, "max_hits": max_hits, "by_keys": {}}
    for K in ks:
        keys = [KEY] + [hashlib.sha256(b"recover_bench key %d" % j).digest() for j in range(1, K)]
        d_keys = torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).to(dev)
        d_am = d_a.repeat(K)
        fsb, ksb = bv.verify_find_workspace_bytes(ms, K), bv.scan_keys_workspace_bytes(ms, K)
        d_fws = torch.empty(fsb, dtype=torch.uint8, device=dev)
        d_kws = torch.empty(ksb, dtype=torch.uint8, device=dev)
        d_stK = torch.full((K, count), 7, dtype=torch.int32, device=dev)
        d_mK = torch.zeros((K, count, 4), dtype=torch.int64, device=dev)
        h_stK = torch.empty((K, count), dtype=torch.int32, pin_memory=True)
        h_mK = torch.empty((K, count, 4), dtype=torch.int64, pin_memory=True)
        got = {}

        def fused():
            bv.verify_find_serialized_mixed_keys_device(d_p.data_ptr(), d_c.data_ptr(), ms, d_keys.data_ptr(), K,
                                                        d_sealed.data_ptr(), d_ok_f.data_ptr(), d_hits.data_ptr(), max_hits,
                                                        d_n.data_ptr(), d_fws.data_ptr(), fsb, st, sealed=True, index_base=BASE)
            h_ok_f.copy_(d_ok_f, non_blocking=True)
            got["n"] = int(d_n.cpu()[0])   # the count first, then as many records
            w = min(got["n"], max_hits)
            h_hits[:w].copy_(d_hits[:w], non_blocking=True)

        def today():
            bv.verify_serialized_mixed_device(d_p.data_ptr(), d_c.data_ptr(), ms, d_ok_t.data_ptr(), d_vws.data_ptr(), vsb, st,
                                              transcript=True)
            bv.scan_serialized_mixed_keys_device(d_p.data_ptr(), d_c.data_ptr(), ms, d_keys.data_ptr(), K, d_mK.data_ptr(),
                                                 d_stK.data_ptr(), d_kws.data_ptr(), ksb, st, index_base=BASE,
                                                 d_amounts=d_am.data_ptr())
            h_ok_t.copy_(d_ok_t, non_blocking=True)
            h_stK.copy_(d_stK, non_blocking=True)
            h_mK.copy_(d_mK, non_blocking=True)

        fns = {"both": [fused, today], "fused": [fused], "today": [today]}[args.side]
        ts = step(900, lambda: alternate(torch, fns, args.reps, args.warmup))
        torch.cuda.synchronize()
        res = {"pairs": K * count, "find_workspace_bytes": fsb, "today_workspace_bytes": vsb + ksb,
               "today_copy_bytes": K * count * 36 + count * 4}
        if args.side in ("both", "fused"):
            hits = h_hits.numpy().view(np.uint32)
            amounts = hits[:, 2].astype(np.uint64) | hits[:, 3].astype(np.uint64) << np.uint64(32)
            res["fused"] = stats(ts[0])
            res["hits_found"] = got["n"]
            res["fused_copy_bytes"] = count * 4 + 4 + min(got["n"], max_hits) * 48
            res["verdicts_all_ok"] = bool((h_ok_f.numpy() == 0).all())
            res["hits_as_expected"] = bool(got["n"] == count and (hits[:, 0] == 0).all() and
                                           (hits[:, 1] == np.arange(count)).all() and
                                           (amounts == d_a.cpu().numpy().view(np.uint64)).all())
        if args.side in ("both", "today"):
            res["today"] = stats(ts[-1])
            status = h_stK.numpy()
            res["status_as_expected"] = bool((status[0] == 0).all() and (status[1:] == 1).all() and (h_ok_t.numpy() == 0).all())
        if args.side == "both":
            res["masks_agree"] = bool((h_hits.numpy()[:, 4:].view(np.uint64).reshape(count, 4) ==
                                       h_mK.numpy()[0].view(np.uint64)).all())
            per_rep = [f / t for f, t in zip(ts[0], ts[1])]
            res["ratio_fused_over_today"] = statistics.median(ts[0]) / statistics.median(ts[1])
            res["ratio_per_rep"] = {"median": statistics.median(per_rep), "min": min(per_rep), "max": max(per_rep)}
        out["find"]["by_keys"][str(K)] = res
        print("find %d" % K, json.dumps(res), flush=True)
        wrong = [c for c in ("verdicts_all_ok", "hits_as_expected", "status_as_expected", "masks_agree") if res.get(c) is False]
        if wrong:   # a run that computed something else is no measurement: recorded as incomplete, non-zero exit
            raise RuntimeError("find leg, K = %d: %s" % (K, ", ".join(wrong)))
        del d_keys, d_am, d_fws, d_kws, d_stK, d_mK, h_stK, h_mK


def view_tag(key, idx):
    """the first byte of SHA-256(key || "bppt" || idx as u64 LE || 0 || 0), by hashlib"""
    return hashlib.sha256(key + b"bppt" + struct.pack("<QII", idx, 0, 0)).digest()[0]


def tags_leg(torch, B, a, bv, ks, args, out):
    """the tagged find call against the untagged one and against the call without keys; key 0 made the block and its tags"""
    ms = block_shapes("wallet", args.scale)
    count = len(ms)
    d_p, d_c, d_a = step(600, lambda: make_block(torch, B, a, bv, ms))
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    d_sealed = torch.zeros_like(d_a)
    bv.seal_amounts_device(KEY, d_a.data_ptr(), count, d_sealed.data_ptr(), st, index_base=BASE)
    d_tags = torch.zeros((count,), dtype=torch.uint8, device=dev)
    bv.view_tags_device(KEY, count, d_tags.data_ptr(), st, index_base=BASE)
    torch.cuda.synchronize()
    tags = d_tags.cpu().numpy()
    probe = list(range(0, count, max(1, count // 64)))
    tags_are_hashlib = all(int(tags[i]) == view_tag(KEY, BASE + i) for i in probe)
    d_ok = torch.full((count,), 7, dtype=torch.int32, device=dev)
    h_ok = torch.empty((count,), dtype=torch.int32, pin_memory=True)
    max_hits = count
    d_hits = torch.zeros((max_hits, 12), dtype=torch.int32, device=dev)
    h_hits = torch.empty((max_hits, 12), dtype=torch.int32, pin_memory=True)
    d_n = torch.zeros((2,), dtype=torch.int32, device=dev)   # hits, candidates
    out["find_tags"] = {"block": "wallet", "count": count, "max_hits": max_hits, "tags_are_hashlib": tags_are_hashlib, "by_keys": {}}
    want_amounts = d_a.cpu().numpy().view(np.uint64)
    for K in ks:
        keys = [KEY] + [hashlib.sha256(b"recover_bench key %d" % j).digest() for j in range(1, K)]
        d_keys = torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).to(dev)
        tsb, fsb = bv.verify_find_tagged_workspace_bytes(ms, K), bv.verify_find_workspace_bytes(ms, K)
        d_ws = torch.empty(tsb, dtype=torch.uint8, device=dev)
        got = {}

        def find(name, nk, wsb, tagged):
            def run():
                d_n.zero_()
                bv.verify_find_serialized_mixed_keys_device(d_p.data_ptr(), d_c.data_ptr(), ms, d_keys.data_ptr() if nk else 0, nk,
                                                            d_sealed.data_ptr() if nk else 0, d_ok.data_ptr(),
                                                            d_hits.data_ptr() if nk else 0, max_hits, d_n.data_ptr(),
                                                            d_ws.data_ptr(), wsb, st, sealed=True, index_base=BASE,
                                                            d_tags=d_tags.data_ptr() if tagged else 0,
                                                            d_n_candidates=d_n.data_ptr() + 4 if tagged else 0)
                h_ok.copy_(d_ok, non_blocking=True)
                got[name] = d_n.cpu().numpy().tolist()   # the counts first, then as many records
                w = min(got[name][0], max_hits)
                h_hits[:w].copy_(d_hits[:w], non_blocking=True)
            return run

        def check(name):
            torch.cuda.synchronize()
            hits = h_hits.numpy().view(np.uint32)
            amounts = hits[:, 2].astype(np.uint64) | hits[:, 3].astype(np.uint64) << np.uint64(32)
            return bool((h_ok.numpy() == 0).all() and got[name][0] == count and (hits[:, 0] == 0).all() and
                        (hits[:, 1] == np.arange(count)).all() and (amounts == want_amounts).all())

        tagged, untagged = find("tagged", K, tsb, True), find("untagged", K, fsb, False)
        no_keys = find("no_keys", 0, bv.verify_find_workspace_bytes(ms, 0), False)
        res = {"pairs": K * count, "tagged_workspace_bytes": tsb, "untagged_workspace_bytes": fsb}
        # each side once alone, so that what is checked is that side's answer
        for name, f in (("untagged", untagged), ("tagged", tagged)):
            h_hits.zero_()
            step(300, f)
            res[name + "_hits_as_expected"] = check(name)
        chance = sum(1 for j in range(1, K) for i in probe if view_tag(keys[j], BASE + i) == int(tags[i]))
        res["n_candidates"] = got["tagged"][1]
        res["candidates_over_pairs"] = got["tagged"][1] / (K * count)
        res["chance_matches_in_probe"] = {"found": chance, "probed_pairs": (K - 1) * len(probe)}
        res["candidates_as_expected"] = bool(count <= got["tagged"][1] <= count + max(64, 2 * (K - 1) * count // 256))
        ts = step(900, lambda: alternate(torch, [tagged, untagged, no_keys], args.reps, args.warmup))
        torch.cuda.synchronize()
        res["tagged"], res["untagged"], res["no_keys"] = stats(ts[0]), stats(ts[1]), stats(ts[2])
        per_rep = [t / u for t, u in zip(ts[0], ts[1])]
        res["ratio_tagged_over_untagged"] = statistics.median(ts[0]) / statistics.median(ts[1])
        res["ratio_per_rep"] = {"median": statistics.median(per_rep), "min": min(per_rep), "max": max(per_rep)}
        res["ratio_tagged_over_no_keys"] = statistics.median(ts[0]) / statistics.median(ts[2])
        res["grows_with_keys_ms"] = {"tagged": statistics.median(ts[0]) - statistics.median(ts[2]),
                                     "untagged": statistics.median(ts[1]) - statistics.median(ts[2])}
        # the acceptance of DESIGN 4l: faster than the untagged call by more than that leg's run-to-run spread
        res["faster_by_more_than_untagged_spread"] = bool(statistics.median(ts[1]) - statistics.median(ts[0]) >
                                                          max(ts[1]) - min(ts[1]))
        out["find_tags"]["by_keys"][str(K)] = res
        print("tags %d" % K, json.dumps(res), flush=True)
        wrong = [c for c in ("untagged_hits_as_expected", "tagged_hits_as_expected", "candidates_as_expected")
                 if res.get(c) is False] + ([] if tags_are_hashlib else ["tags_are_hashlib"])
        if wrong:   # a run that computed something else is no measurement
            raise RuntimeError("tags leg, K = %d: %s" % (K, ", ".join(wrong)))
        del d_keys, d_ws


def output_tag(key, idx, j):
    """the first byte of SHA-256(key || "bppt" || idx as u64 LE || j as u32 LE || 0), by hashlib"""
    return hashlib.sha256(key + b"bppt" + struct.pack("<QII", idx, j, 0)).digest()[0]


def outputs_leg(torch, B, a, bv, ks, args, out):
    """the per-output find call on containers of m = 4 against the tagged find call on the wallet block of as many single
    outputs, each also with n_keys = 0; key 0 owns every output of both blocks and made their tags"""
    M = 4
    ms1 = block_shapes("wallet", args.scale)
    n_out = len(ms1) // M * M
    ms1 = ms1[:n_out]
    ms4 = np.full(n_out // M, M, dtype=np.uint32)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    # the wallet block, sealed and tagged by the existing calls
    d_p1, d_c1, d_a1 = step(600, lambda: make_block(torch, B, a, bv, ms1))
    d_sealed1 = torch.zeros_like(d_a1)
    bv.seal_amounts_device(KEY, d_a1.data_ptr(), n_out, d_sealed1.data_ptr(), st, index_base=BASE)
    d_tags1 = torch.zeros((n_out,), dtype=torch.uint8, device=dev)
    bv.view_tags_device(KEY, n_out, d_tags1.data_ptr(), st, index_base=BASE)
    # the block of aggregated proofs: masks, sealed amounts and tags by the sender's call under key 0, proofs under a sender key
    rng = np.random.default_rng(13)
    vals = rng.integers(0, 1 << 31, size=n_out, dtype=np.uint64)
    d_v = torch.from_numpy(vals.view(np.int64)).to(dev)
    d_ok_keys = torch.from_numpy(np.frombuffer(KEY * n_out, dtype=np.uint8).copy()).to(dev)
    d_ix = torch.from_numpy((np.uint64(BASE) + np.arange(n_out, dtype=np.uint64) // np.uint64(M)).view(np.int64)).to(dev)
    d_j = torch.from_numpy((np.arange(n_out, dtype=np.uint32) % M).view(np.int32)).to(dev)
    d_g = torch.zeros((n_out, 4), dtype=torch.int64, device=dev)
    d_sealed4 = torch.zeros((n_out,), dtype=torch.int64, device=dev)
    d_tags4 = torch.zeros((n_out,), dtype=torch.uint8, device=dev)
    bv.make_outputs_device(d_ok_keys.data_ptr(), d_ix.data_ptr(), d_j.data_ptr(), d_v.data_ptr(), n_out, d_g.data_ptr(),
                           d_sealed4.data_ptr(), d_tags4.data_ptr(), st)
    pb = B.compressed_bytes(a)
    d_p4 = torch.zeros(len(ms4) * B.proof_bytes(a, N, M), dtype=torch.uint8, device=dev)
    d_c4 = torch.zeros(n_out * pb, dtype=torch.uint8, device=dev)
    wsb = bv.prover_mixed_workspace_bytes(ms4, serialized=True)
    d_pws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    sender = hashlib.sha256(b"recover_bench sender").digest()
    step(600, lambda: (bv.prove_serialized_mixed_device(d_v.data_ptr(), d_g.data_ptr(), ms4, d_p4.data_ptr(), d_c4.data_ptr(),
                                                        d_pws.data_ptr(), wsb, st, transcript=True, blind_key=sender,
                                                        index_base=BASE), torch.cuda.synchronize()))
    del d_pws, d_ok_keys
    tags4 = d_tags4.cpu().numpy()
    tags_are_hashlib = all(int(tags4[o]) == output_tag(KEY, BASE + o // M, o % M) for o in range(0, n_out, max(1, n_out // 256)))
    max_hits = n_out
    d_ok = torch.full((n_out,), 7, dtype=torch.int32, device=dev)
    h_ok = torch.empty((n_out,), dtype=torch.int32, pin_memory=True)
    d_hits = torch.zeros((max_hits, 12), dtype=torch.int32, device=dev)
    h_hits = torch.empty((max_hits, 12), dtype=torch.int32, pin_memory=True)
    d_n = torch.zeros((2,), dtype=torch.int32, device=dev)   # hits, candidates
    out["find_outputs"] = {"outputs": n_out, "m": M, "containers": len(ms4), "single_block": "wallet", "max_hits": max_hits,
                           "tags_are_hashlib": tags_are_hashlib, "by_keys": {}}
    want = {"outputs": vals, "tagged": d_a1.cpu().numpy().view(np.uint64)}
    for K in ks:
        keys = [KEY] + [hashlib.sha256(b"recover_bench key %d" % j).digest() for j in range(1, K)]
        d_keys = torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).to(dev)
        osb, tsb = bv.verify_find_outputs_workspace_bytes(ms4, K), bv.verify_find_tagged_workspace_bytes(ms1, K)
        d_ws = torch.empty(max(osb, tsb), dtype=torch.uint8, device=dev)
        got = {}

        def finish(name, count):
            h_ok[:count].copy_(d_ok[:count], non_blocking=True)
            got[name] = d_n.cpu().numpy().tolist()   # the counts first, then as many records
            w = min(got[name][0], max_hits)
            h_hits[:w].copy_(d_hits[:w], non_blocking=True)

        def outputs(name, nk):
            def run():
                d_n.zero_()
                bv.verify_find_outputs_serialized_mixed_keys_device(
                    d_p4.data_ptr(), d_c4.data_ptr(), ms4, d_keys.data_ptr() if nk else 0, nk, d_sealed4.data_ptr() if nk else 0,
                    d_tags4.data_ptr() if nk else 0, d_ok.data_ptr(), d_hits.data_ptr() if nk else 0, max_hits, d_n.data_ptr(),
                    d_ws.data_ptr(), osb, st, index_base=BASE, d_n_candidates=d_n.data_ptr() + 4)
                finish(name, len(ms4))
            return run

        def tagged(name, nk):
            def run():
                d_n.zero_()
                bv.verify_find_serialized_mixed_keys_device(d_p1.data_ptr(), d_c1.data_ptr(), ms1, d_keys.data_ptr() if nk else 0, nk,
                                                            d_sealed1.data_ptr() if nk else 0, d_ok.data_ptr(),
                                                            d_hits.data_ptr() if nk else 0, max_hits, d_n.data_ptr(),
                                                            d_ws.data_ptr(), tsb, st, sealed=True, index_base=BASE,
                                                            d_tags=d_tags1.data_ptr() if nk else 0,
                                                            d_n_candidates=d_n.data_ptr() + 4 if nk else 0)
                finish(name, n_out)
            return run

        def check(name, count):
            torch.cuda.synchronize()
            hits = h_hits.numpy().view(np.uint32)
            amounts = hits[:, 2].astype(np.uint64) | hits[:, 3].astype(np.uint64) << np.uint64(32)
            return bool((h_ok.numpy()[:count] == 0).all() and got[name][0] == n_out and (hits[:, 0] == 0).all() and
                        (hits[:, 1] == np.arange(n_out)).all() and (amounts == want[name]).all())

        fns = [outputs("outputs", K), tagged("tagged", K), outputs("outputs_no_keys", 0), tagged("tagged_no_keys", 0)]
        res = {"pairs": K * n_out, "outputs_workspace_bytes": osb, "tagged_workspace_bytes": tsb}
        for name, f, count in (("tagged", fns[1], n_out), ("outputs", fns[0], len(ms4))):   # each once alone: that side's answer
            h_hits.zero_()
            step(300, f)
            res[name + "_hits_as_expected"] = check(name, count)
        # the candidate count of the new call against hashlib, every pair of the foreign keys
        chance = sum(1 for k in keys[1:] for o in range(n_out) if output_tag(k, BASE + o // M, o % M) == int(tags4[o]))
        res["n_candidates"] = got["outputs"][1]
        res["n_candidates_hashlib"] = n_out + chance
        res["candidates_as_expected"] = bool(got["outputs"][1] == n_out + chance)
        res["tagged_n_candidates"] = got["tagged"][1]
        ts = step(900, lambda: alternate(torch, fns, args.reps, args.warmup))
        torch.cuda.synchronize()
        for name, t in zip(("outputs", "tagged", "outputs_no_keys", "tagged_no_keys"), ts):
            res[name] = stats(t)
        med = [statistics.median(t) for t in ts]
        key_part = {"outputs": med[0] - med[2], "tagged": med[1] - med[3]}
        res["key_dependent_ms"] = key_part
        res["key_dependent_per_rep"] = {"outputs": stats([x - y for x, y in zip(ts[0], ts[2])]),
                                        "tagged": stats([x - y for x, y in zip(ts[1], ts[3])])}
        spread = max(max(t) - min(t) for t in ts)
        res["spread_between_repetitions_ms"] = spread
        # the expectation of DESIGN 4m, not a gate
        res["outputs_key_part_within_spread_of_tagged"] = bool(key_part["outputs"] <= key_part["tagged"] + spread)
        out["find_outputs"]["by_keys"][str(K)] = res
        print("outputs %d" % K, json.dumps(res), flush=True)
        wrong = [c for c in ("tagged_hits_as_expected", "outputs_hits_as_expected", "candidates_as_expected")
                 if res.get(c) is False] + ([] if tags_are_hashlib else ["tags_are_hashlib"])
        if wrong:   # a run that computed something else is no measurement
            raise RuntimeError("outputs leg, K = %d: %s" % (K, ", ".join(wrong)))
        del d_keys, d_ws


def merge_kernel_stats(args):
    """folds rocprofv3 k_kernel_stats.csv files (one per side) into the JSON at --out: no GPU"""
    with open(args.out) as f:
        out = json.load(f)
    split = {}
    for item in args.kernel_stats.split(","):
        side, path = item.split("=", 1)
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
        split[side] = [{"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) * 1e-6,
                        "average_us": float(r["AverageNs"]) * 1e-3, "percent": float(r["Percentage"])} for r in rows
                       if float(r["Percentage"]) >= 0.1]
    leg = "find" if set(split) <= {"fused", "today"} else "keys"
    out.setdefault(leg, {})["kernel_split"] = split
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"merged": sorted(split), "out": args.out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", default="")
    ap.add_argument("--find", action="store_true")
    ap.add_argument("--tags", action="store_true")
    ap.add_argument("--outputs", action="store_true")
    ap.add_argument("--side", default="both", choices=("both", "many", "single", "fused", "today"))
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=int, default=13)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--legs", default="sr")
    ap.add_argument("--blocks", default="mixed,wallet")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recover_bench.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args)
    if args.find:
        # --find: that leg alone, at --keys; with --tags the tagged call's, with --outputs the per-output call's
        args.legs = "o" if args.outputs else "t" if args.tags else "f"
    elif args.keys and "k" not in args.legs:
        args.legs = "k"   # --keys alone: the many-key leg alone
    import torch
    import bulletproofsplus_amd as B
    a = B.Arith("bls12_381")
    bv = step(300, lambda: B.BatchVerifier(B.PublicKey.new(a, N * CAP), N, CAP, window_bits=args.window))
    out = {"curve": "bls12_381", "n": N, "capacity_m": CAP, "window_bits": args.window, "reps": args.reps, "warmup": args.warmup,
           "scale": args.scale, "device": torch.cuda.get_device_name(0), "scan": {}, "recover": {}, "complete": False}
    try:
        if "s" in args.legs:
            for name in args.blocks.split(","):
                scan_leg(torch, B, a, bv, name, args, out)
        if "r" in args.legs:
            for log2n in (12, 16):
                recover_leg(torch, B, a, bv, log2n, args, out)
        if "k" in args.legs:
            keys_leg(torch, B, a, bv, [int(x) for x in (args.keys or "1,4,16,64").split(",")], args, out)
        if "f" in args.legs:
            find_leg(torch, B, a, bv, [int(x) for x in (args.keys or "1,16,64").split(",")], args, out)
        if "t" in args.legs:
            tags_leg(torch, B, a, bv, [int(x) for x in (args.keys or "1,16,64,256").split(",")], args, out)
        if "o" in args.legs:
            outputs_leg(torch, B, a, bv, [int(x) for x in (args.keys or "16,64,256").split(",")], args, out)
        out["complete"] = True
    except StepTimeout:
        out["stopped"] = "a step ran into its time limit"
    finally:
        complete = out["complete"]
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        if args.find and os.path.exists(args.out):   # beside what the other legs recorded there
            with open(args.out) as f:
                kept = json.load(f)
            leg = "find_outputs" if args.outputs else "find_tags" if args.tags else "find"
            kept[leg] = dict(out.get(leg, {}), reps=args.reps, warmup=args.warmup, window_bits=args.window,
                             scale=args.scale, device=out["device"], complete=out["complete"])
            out = kept
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps({"complete": complete, "out": args.out}))


if __name__ == "__main__":
    main()
