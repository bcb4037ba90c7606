#!/usr/bin/env python3
"""A block of range proofs with mixed aggregation sizes, verified by ONE verifier (bpp_verifier_run_mixed) against the
same proofs verified class by class on dedicated verifiers (bpp_verifier_run).

The block: BLS12-381, n = 64, capacity m = 16, window 16; 8 192 distinct proofs made on the device by the batched
prover, m_i distributed 4096 / 2048 / 1024 / 512 / 512 over m_i = 1 / 2 / 4 / 8 / 16, shuffled, a handful with a flipped
s'.  Prints one JSON object: both times (device events, after warm-up) with their spread, their ratio, verifies/s of the
mixed block, the table bytes of the one verifier against the sum of the dedicated ones, and whether the verdict vectors
are identical.
usage: python tools/mixed_bench.py [--reps 20] [--warmup 3] [--window 16] [--out profiles/mixed_bench.json]
       [--mixed-only]   (no dedicated verifiers: the run to put under rocprofv3 --kernel-trace --stats)
       [--serialized]   the same block as BYTES: proofs made under the transcript, encoded as containers, and verified by
                        bpp_range_verify_batch_serialized_mixed_device (one call) against five
                        bpp_range_verify_batch_serialized_device calls on the dedicated verifiers, the two ALTERNATED
                        repetition by repetition; also, timed by the wall clock, the host-side detour the one call
                        replaces (decode per class, re-pack wire records, derive_challenges_mixed + run_mixed).
                        Write it with --out profiles/mixed_serialized_bench.json
       [--grouped]      the GROUPED check over the same block (bpp_verifier_run_grouped_mixed; with --serialized
                        bpp_range_verify_batch_serialized_grouped_mixed_device), subgroup check on.  Four legs, alternated
                        repetition by repetition, the verdict / status vectors compared after each:
                          A  the new call on the all-valid block
                          B  the exact mixed call on the same buffers
                          C  five grouped calls on the dedicated verifiers, the proofs pre-sorted by class
                          A' the new call on the block with --tamper proofs flipped
                        Write it with --out profiles/mixed_grouped_bench.json / mixed_grouped_serialized_bench.json;
                        with --mixed-only: leg A alone (the run to put under rocprofv3 --kernel-trace --stats)
       [--prove]        PROVING the same block of values, under the transcript (literal blinding), as containers in HBM.
                        Three legs, alternated repetition by repetition:
                          A  one bpp_range_prove_batch_serialized_mixed_device call on the capacity engine
                          B  five bpp_range_prove_batch_fs_device calls on dedicated engines, the inputs pre-sorted by class
                          C  (wall clock) what a caller did after B to get the same bytes: D2H, bpp_proofs_encode_version
                             and bpp_points_compress per class, the interleave into caller order
                        A's bytes are compared with C's after every repetition.  Write it with
                        --out profiles/mixed_prove_bench.json; with --mixed-only: leg A alone, one engine, no comparison"""
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


def timed(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--tamper", type=int, default=8, help="proofs with a flipped s'")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--mixed-only", action="store_true")
    ap.add_argument("--serialized", action="store_true")
    ap.add_argument("--grouped", action="store_true")
    ap.add_argument("--prove", action="store_true")
    ap.add_argument("--group", type=int, default=32)
    ap.add_argument("--detour-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bulletproofsplus_amd as B
    dev = torch.device("cuda:0")
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    rng = np.random.default_rng(args.seed)
    a = B.Arith("bls12_381")
    pk = B.PublicKey.new(a, N * CAP)
    t0 = time.time()
    cap = B.BatchVerifier(pk, N, CAP, window_bits=args.window)
    build_s = {"capacity": time.time() - t0}
    if args.prove:
        return prove(args, torch, B, a, cap, rng, build_s)
    # engines that make (and, for the comparison, verify) each class's proofs: the dedicated (64, m') verifiers
    ded = {}
    for m in MIX:
        if m == CAP:
            ded[m] = cap
        elif not args.mixed_only:
            t0 = time.time()
            ded[m] = B.BatchVerifier(B.PublicKey.new(a, N * m), N, m, window_bits=args.window)
            build_s[str(m)] = time.time() - t0
        else:
            ded[m] = B.BatchVerifier(B.PublicKey.new(a, N * m), N, m, window_bits=8)   # a prover only
    recs, scs = {}, {}
    for m, cnt in MIX.items():
        # values below 2^31 (RangeProver::commit takes v as i32); every proof distinct
        vals = rng.integers(0, 1 << 31, size=(cnt, m), dtype=np.uint64)
        gams = rng.integers(1, 1 << 62, size=(cnt, m, 4), dtype=np.uint64)
        gams[:, :, 1:] = 0
        pts, sc, V = ded[m].prove_batch(vals, gams, transcript=args.serialized)
        recs[m] = np.concatenate([pts, V], axis=1)
        scs[m] = sc
    if args.mixed_only:
        for m in MIX:
            if m != CAP:
                ded[m].close()
    # the block in caller order: shuffled, a handful tampered
    order = [(m, i) for m, cnt in MIX.items() for i in range(cnt)]
    perm = rng.permutation(len(order))
    order = [order[p] for p in perm]
    victims = [int(t) for t in rng.choice(len(order), size=args.tamper, replace=False)]
    count = len(order)
    ms = [m for m, _ in order]
    if args.grouped:
        return grouped(args, torch, B, a, cap, ded, recs, scs, order, ms, victims, build_s)
    for t in victims:
        m, i = order[t]
        scs[m][i, 1, 0] ^= 1
    if args.serialized:
        return serialized(args, torch, B, a, cap, ded, recs, scs, order, ms, build_s)
    packed = np.ascontiguousarray(np.concatenate([recs[m][i] for m, i in order]))
    d_pts = torch.from_numpy(packed.view(np.int64)).to(dev)
    d_sc = torch.from_numpy(np.ascontiguousarray(np.stack([scs[m][i] for m, i in order])).view(np.int64)).to(dev)
    d_ok = torch.full((count,), 7, dtype=torch.int32, device=dev)
    wsb = cap.mixed_workspace_bytes(ms)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def mixed():
        cap.run_mixed_device(d_pts.data_ptr(), d_sc.data_ptr(), ms, d_ok.data_ptr(), d_ws.data_ptr(), wsb, stream())

    t_mixed = timed(torch, mixed, args.reps, args.warmup)
    ok_mixed = d_ok.cpu().numpy().astype(np.uint32)
    res = {"shape": {"curve": "bls12_381", "n": N, "capacity_m": CAP, "window": args.window, "count": count,
                     "mix": {str(m): c for m, c in MIX.items()}, "tampered": args.tamper},
           "mixed": stats(t_mixed), "mixed_verifies_per_s": count / (statistics.median(t_mixed) / 1e3),
           "mixed_rejects": int(ok_mixed.sum()), "table_bytes_one": int(cap.table_bytes),
           "mixed_workspace_bytes": int(wsb), "build_s": build_s}
    if not args.mixed_only:
        # the same proofs, class by class on the dedicated verifiers (class-contiguous buffers prepared up front)
        pos = {m: [j for j, (mm, _) in enumerate(order) if mm == m] for m in MIX}
        bufs = {}
        for m in MIX:
            cnt = len(pos[m])
            r = np.ascontiguousarray(np.stack([recs[m][order[j][1]] for j in pos[m]]))
            s = np.ascontiguousarray(np.stack([scs[m][order[j][1]] for j in pos[m]]))
            w = ded[m].workspace_bytes(cnt)
            bufs[m] = (torch.from_numpy(r.view(np.int64)).to(dev), torch.from_numpy(s.view(np.int64)).to(dev),
                       torch.full((cnt,), 7, dtype=torch.int32, device=dev), torch.empty(w, dtype=torch.uint8, device=dev),
                       w, cnt)

        def dedicated():
            for m in MIX:
                p, s, o, w, wb, cnt = bufs[m]
                ded[m].run_device(p.data_ptr(), s.data_ptr(), cnt, o.data_ptr(), w.data_ptr(), wb, stream())

        t_ded = timed(torch, dedicated, args.reps, args.warmup)
        ok_ded = np.zeros(count, dtype=np.uint32)
        per_class = {}
        for m in MIX:
            ok_ded[pos[m]] = bufs[m][2].cpu().numpy().astype(np.uint32)
            p, s, o, w, wb, cnt = bufs[m]
            one = timed(torch, lambda: ded[m].run_device(p.data_ptr(), s.data_ptr(), cnt, o.data_ptr(), w.data_ptr(), wb,
                                                         stream()), max(5, args.reps // 2), 1)
            per_class[str(m)] = statistics.median(one)
        res.update({"dedicated": stats(t_ded), "dedicated_per_class_median_ms": per_class,
                    "ratio_mixed_over_dedicated": statistics.median(t_mixed) / statistics.median(t_ded),
                    "table_bytes_dedicated_sum": int(sum(ded[m].table_bytes for m in MIX)),
                    "verdicts_identical": bool(np.array_equal(ok_mixed, ok_ded))})
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def serialized(args, torch, B, a, cap, ded, recs, scs, order, ms, build_s):
    """the --serialized leg: the block as containers in HBM, transcript on"""
    dev = torch.device("cuda:0")
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    count = len(order)
    blobs, comms = {}, {}
    for m in MIX:
        k = (N * m).bit_length() - 1
        blobs[m] = B.encode_proofs(a, N, m, recs[m][:, :3 + 2 * k], scs[m])
        comms[m] = B.compress_points(a, recs[m][:, 3 + 2 * k:].reshape(-1, a.PW)).reshape(len(recs[m]), -1)
    raw = np.concatenate([blobs[m][i] for m, i in order])
    cm = np.concatenate([comms[m][i] for m, i in order])
    assert B.proofs_scan(a, N, raw).tolist() == ms
    d_raw, d_cm = torch.from_numpy(raw).to(dev), torch.from_numpy(cm).to(dev)
    d_ok = torch.full((count,), 7, dtype=torch.int32, device=dev)
    wsb = cap.serialized_mixed_workspace_bytes(ms)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def one_call():
        cap.verify_serialized_mixed_device(d_raw.data_ptr(), d_cm.data_ptr(), ms, d_ok.data_ptr(), d_ws.data_ptr(), wsb,
                                           stream(), transcript=True)

    res = {"shape": {"curve": "bls12_381", "n": N, "capacity_m": CAP, "window": args.window, "count": count,
                     "mix": {str(m): c for m, c in MIX.items()}, "tampered": args.tamper, "transcript": True,
                     "container_bytes": int(len(raw)), "commitment_bytes": int(len(cm))},
           "table_bytes_one": int(cap.table_bytes), "serialized_mixed_workspace_bytes": int(wsb), "build_s": build_s}
    if args.mixed_only:
        t_one = timed(torch, one_call, args.reps, args.warmup)
        res.update({"serialized_mixed": stats(t_one), "rejects": int((d_ok.cpu().numpy() != 0).sum())})
        return finish(args, res)
    pos = {m: [j for j, (mm, _) in enumerate(order) if mm == m] for m in MIX}
    bufs = {}
    for m in MIX:
        idx = [order[j][1] for j in pos[m]]
        cnt = len(idx)
        w = ded[m].serialized_workspace_bytes(cnt)
        bufs[m] = (torch.from_numpy(np.ascontiguousarray(blobs[m][idx])).to(dev),
                   torch.from_numpy(np.ascontiguousarray(comms[m][idx])).to(dev),
                   torch.full((cnt,), 7, dtype=torch.int32, device=dev), torch.empty(w, dtype=torch.uint8, device=dev), w, cnt)

    def five_calls():
        for m in MIX:
            p, c, o, w, wb, cnt = bufs[m]
            ded[m].verify_serialized_device(p.data_ptr(), c.data_ptr(), cnt, o.data_ptr(), w.data_ptr(), wb, stream(),
                                            transcript=True)

    # alternated on one box: one repetition of each, in turn
    for _ in range(args.warmup):
        one_call()
        five_calls()
    torch.cuda.synchronize()
    t_one, t_five = [], []
    for _ in range(args.reps):
        t_one += timed(torch, one_call, 1, 0)
        t_five += timed(torch, five_calls, 1, 0)
    ok_one = d_ok.cpu().numpy().astype(np.uint32)
    ok_five = np.zeros(count, dtype=np.uint32)
    for m in MIX:
        ok_five[pos[m]] = bufs[m][2].cpu().numpy().astype(np.uint32)
    res.update({"serialized_mixed": stats(t_one), "dedicated_serialized": stats(t_five),
                "ratio_mixed_over_dedicated": statistics.median(t_one) / statistics.median(t_five),
                "serialized_mixed_verifies_per_s": count / (statistics.median(t_one) / 1e3),
                "rejects": int((ok_one != 0).sum()), "format_errors": int((ok_one == 2).sum()),
                "table_bytes_dedicated_sum": int(sum(ded[m].table_bytes for m in MIX)),
                "status_vectors_identical": bool(np.array_equal(ok_one, ok_five))})
    # the "before": what a user of this library did with such a block -- decode each class on its own, re-pack the wire
    # records in caller order, then the unserialized mixed call under the transcript.  Host work: timed by the wall clock.
    if args.detour_reps:
        nch = [3 + (N * m).bit_length() - 1 for m in ms]
        w2 = cap.mixed_workspace_bytes(ms)
        d_ws2 = torch.empty(w2, dtype=torch.uint8, device=dev)
        d_ch = torch.zeros(sum(nch) * 4, dtype=torch.int64, device=dev)
        d_ok2 = torch.full((count,), 7, dtype=torch.int32, device=dev)
        lens = [len(blobs[m][0]) for m in ms]
        starts = np.concatenate([[0], np.cumsum(lens)])
        clens = [len(comms[m][0]) for m in ms]
        cstarts = np.concatenate([[0], np.cumsum(clens)])
        t_detour = []
        for _ in range(args.detour_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            status = np.zeros(count, dtype=np.uint32)
            rec_of, sc_of = [None] * count, [None] * count
            for m in MIX:
                sel = pos[m]
                pb = np.stack([raw[starts[j]:starts[j + 1]] for j in sel])
                pts, sc, st = B.decode_proofs(a, N, m, pb)
                V, vok = B.decompress_points(a, np.stack([cm[cstarts[j]:cstarts[j + 1]] for j in sel]).reshape(-1, comms[m].shape[1] // m))
                V = V.reshape(len(sel), m, a.PW)
                st = st | (2 * (vok.reshape(len(sel), m).max(axis=1) != 0)).astype(np.uint32)
                for t, j in enumerate(sel):
                    rec_of[j] = np.concatenate([pts[t], V[t]])
                    sc_of[j] = sc[t]
                    status[j] = st[t]
            d_pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(rec_of)).view(np.int64)).to(dev)
            d_sc = torch.from_numpy(np.ascontiguousarray(np.stack(sc_of)).view(np.int64)).to(dev)
            cap.derive_challenges_mixed_device(d_pts.data_ptr(), ms, d_ch.data_ptr(), d_ws2.data_ptr(), w2, stream())
            cap.run_mixed_device(d_pts.data_ptr(), d_sc.data_ptr(), ms, d_ok2.data_ptr(), d_ws2.data_ptr(), w2, stream(),
                                 d_challenges=d_ch.data_ptr())
            ok2 = d_ok2.cpu().numpy().astype(np.uint32)
            ok2[status != 0] = 2
            t_detour.append((time.perf_counter() - t0) * 1e3)
        res.update({"host_detour_wall": stats(t_detour), "host_detour_statuses_identical": bool(np.array_equal(ok2, ok_one))})
    return finish(args, res)


def grouped(args, torch, B, a, cap, ded, recs, scs, order, ms, victims, build_s):
    """the --grouped legs (wire records, or with --serialized containers under the transcript)"""
    dev = torch.device("cuda:0")
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    count, group, ser = len(order), args.group, args.serialized
    key = os.urandom(32)
    # the condition the header states for the weighted checks: prime-order points.  Wire records: the subgroup check of the
    # pass, on for every leg; containers: the decoder's own membership test provides it
    for v in ([cap] if args.mixed_only else set(ded.values())):
        v.set_subgroup_check(not ser)
    gof = B.mixed_groups(ms, group)
    want_bad = np.zeros(count, dtype=np.uint32)
    want_bad[victims] = 1
    hit = sorted(set(gof[victims].tolist()))
    want_stats = (len(hit), int(sum(int((gof == h).sum()) for h in hit)))

    def tampered(m):
        sc = scs[m].copy()
        for t in victims:
            if order[t][0] == m:
                sc[order[t][1], 1, 0] ^= 1
        return sc
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    if ser:
        blobs, blobs_bad, comms = {}, {}, {}
        for m in MIX:
            k = (N * m).bit_length() - 1
            blobs[m] = B.encode_proofs(a, N, m, recs[m][:, :3 + 2 * k], scs[m])
            blobs_bad[m] = B.encode_proofs(a, N, m, recs[m][:, :3 + 2 * k], tampered(m))
            comms[m] = B.compress_points(a, recs[m][:, 3 + 2 * k:].reshape(-1, a.PW)).reshape(len(recs[m]), -1)
        d_in = up(np.concatenate([blobs[m][i] for m, i in order]))
        d_in_bad = up(np.concatenate([blobs_bad[m][i] for m, i in order]))
        d_aux = up(np.concatenate([comms[m][i] for m, i in order]))
        wsb = cap.serialized_grouped_mixed_workspace_bytes(ms, group)
        wsb_exact = cap.serialized_mixed_workspace_bytes(ms)
    else:
        d_in = up(np.concatenate([recs[m][i] for m, i in order]).view(np.int64))
        d_aux = up(np.stack([scs[m][i] for m, i in order]).view(np.int64))
        bad = {m: tampered(m) for m in MIX}
        d_aux_bad = up(np.stack([bad[m][i] for m, i in order]).view(np.int64))
        wsb = cap.grouped_mixed_workspace_bytes(ms, group)
        wsb_exact = cap.mixed_workspace_bytes(ms)
    d_ws = torch.empty(max(wsb, wsb_exact), dtype=torch.uint8, device=dev)
    d_ok = {leg: torch.full((count,), 7, dtype=torch.int32, device=dev) for leg in ("A", "B", "A_tampered")}
    got_stats = {}

    def leg_a(which="A"):
        if ser:
            got_stats[which] = cap.verify_serialized_grouped_mixed_device(
                (d_in if which == "A" else d_in_bad).data_ptr(), d_aux.data_ptr(), ms, d_ok[which].data_ptr(), d_ws.data_ptr(), wsb,
                key, 0, group, stream(), transcript=True)
        else:
            got_stats[which] = cap.run_grouped_mixed_device(
                d_in.data_ptr(), (d_aux if which == "A" else d_aux_bad).data_ptr(), ms, key, 0, d_ok[which].data_ptr(),
                d_ws.data_ptr(), wsb, group=group, stream=stream())

    def leg_b():
        if ser:
            cap.verify_serialized_mixed_device(d_in.data_ptr(), d_aux.data_ptr(), ms, d_ok["B"].data_ptr(), d_ws.data_ptr(),
                                               wsb_exact, stream(), transcript=True)
        else:
            cap.run_mixed_device(d_in.data_ptr(), d_aux.data_ptr(), ms, d_ok["B"].data_ptr(), d_ws.data_ptr(), wsb_exact, stream())

    res = {"shape": {"curve": "bls12_381", "n": N, "capacity_m": CAP, "window": args.window, "count": count,
                     "mix": {str(m): c for m, c in MIX.items()}, "tampered": args.tamper, "group": group,
                     "groups": int(gof.max()) + 1, "serialized": ser, "transcript": ser, "subgroup_check": not ser},
           "device": torch.cuda.get_device_name(0), "table_bytes_one": int(cap.table_bytes),
           "grouped_mixed_workspace_bytes": int(wsb), "exact_mixed_workspace_bytes": int(wsb_exact), "build_s": build_s}
    if args.mixed_only:
        t_a = timed(torch, leg_a, args.reps, args.warmup)
        res.update({"A_grouped_mixed_valid": stats(t_a), "A_stats": got_stats["A"],
                    "A_all_valid": not bool(d_ok["A"].cpu().numpy().any())})
        return finish(args, res)
    # leg C: the block sorted by class on the host beforehand, one grouped call per dedicated verifier
    pos = {m: [j for j, (mm, _) in enumerate(order) if mm == m] for m in MIX}
    bufs = {}
    for m in MIX:
        idx = [order[j][1] for j in pos[m]]
        cnt = len(idx)
        if ser:
            w = ded[m].serialized_grouped_workspace_bytes(cnt, group)
            first, second = up(blobs[m][idx]), up(comms[m][idx])
        else:
            w = ded[m].grouped_workspace_bytes(cnt, group)
            first, second = up(recs[m][idx].view(np.int64)), up(scs[m][idx].view(np.int64))
        bufs[m] = (first, second, torch.full((cnt,), 7, dtype=torch.int32, device=dev),
                   torch.empty(w, dtype=torch.uint8, device=dev), w, cnt)

    def leg_c():
        for m in MIX:
            p, s, o, w, wb, cnt = bufs[m]
            if ser:
                ded[m].verify_serialized_grouped_device(p.data_ptr(), s.data_ptr(), cnt, o.data_ptr(), w.data_ptr(), wb, key, 0,
                                                        group, stream(), transcript=True)
            else:
                ded[m].run_grouped_device(p.data_ptr(), s.data_ptr(), cnt, key, 0, o.data_ptr(), w.data_ptr(), wb, group=group,
                                          stream=stream())

    legs = (("A", leg_a), ("B", leg_b), ("C", leg_c), ("A_tampered", lambda: leg_a("A_tampered")))
    for _ in range(args.warmup):
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in legs}
    same = {name: True for name, _ in legs}
    for _ in range(args.reps):      # alternated on one box: one repetition of each leg, in turn, its vector checked after it
        for name, fn in legs:
            times[name] += timed(torch, fn, 1, 0)
            if name == "C":
                vec = np.zeros(count, dtype=np.uint32)
                for m in MIX:
                    vec[pos[m]] = bufs[m][2].cpu().numpy().astype(np.uint32)
            else:
                vec = d_ok[name].cpu().numpy().astype(np.uint32)
            same[name] &= bool(np.array_equal(vec, want_bad if name == "A_tampered" else np.zeros(count, dtype=np.uint32)))
            if name in got_stats:
                same[name] &= tuple(got_stats[name]) == (want_stats if name == "A_tampered" else (0, 0))
    med = {name: statistics.median(t) for name, t in times.items()}
    res.update({"A_grouped_mixed_valid": stats(times["A"]), "B_exact_mixed_valid": stats(times["B"]),
                "C_five_grouped_dedicated_valid": stats(times["C"]), "A_grouped_mixed_tampered": stats(times["A_tampered"]),
                "vectors_and_stats_as_expected": same, "A_tampered_stats": list(got_stats["A_tampered"]),
                "A_tampered_stats_predicted": list(want_stats),
                "ratio_A_over_B": med["A"] / med["B"], "ratio_A_over_C": med["A"] / med["C"],
                "ranges_A_B_disjoint": max(times["A"]) < min(times["B"]),
                "A_verifies_per_s": count / (med["A"] / 1e3), "A_tampered_verifies_per_s": count / (med["A_tampered"] / 1e3),
                "table_bytes_dedicated_sum": int(sum(ded[m].table_bytes for m in MIX))})
    return finish(args, res)


def prove(args, torch, B, a, cap, rng, build_s):
    """the --prove legs: the block's values in HBM in, containers and commitments in HBM out"""
    dev = torch.device("cuda:0")
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    order = [(m, i) for m, cnt in MIX.items() for i in range(cnt)]
    order = [order[p] for p in rng.permutation(len(order))]
    count, ms = len(order), [m for m, _ in order]
    vals = {m: rng.integers(0, 1 << 31, size=(cnt, m), dtype=np.uint64) for m, cnt in MIX.items()}
    gams = {m: np.zeros((cnt, m, 4), dtype=np.uint64) for m, cnt in MIX.items()}
    for m in MIX:
        gams[m][:, :, 0] = rng.integers(1, 1 << 62, size=gams[m].shape[:2], dtype=np.uint64)
    d_v = up(np.concatenate([vals[m][i] for m, i in order]).view(np.int64))
    d_g = up(np.concatenate([gams[m][i] for m, i in order]).view(np.int64))
    pbytes = sum(B.proof_bytes(a, N, m) for m in ms)
    cbytes = sum(ms) * B.compressed_bytes(a)
    d_raw = torch.zeros(pbytes, dtype=torch.uint8, device=dev)
    d_cm = torch.zeros(cbytes, dtype=torch.uint8, device=dev)
    wsb = cap.prover_mixed_workspace_bytes(ms, serialized=True)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def leg_a():
        cap.prove_serialized_mixed_device(d_v.data_ptr(), d_g.data_ptr(), ms, d_raw.data_ptr(), d_cm.data_ptr(), d_ws.data_ptr(),
                                          wsb, stream(), transcript=True)

    res = {"shape": {"curve": "bls12_381", "n": N, "capacity_m": CAP, "window": args.window, "count": count,
                     "mix": {str(m): c for m, c in MIX.items()}, "transcript": True, "blinding": "literals",
                     "container_bytes": int(pbytes), "commitment_bytes": int(cbytes)},
           "device": torch.cuda.get_device_name(0), "table_bytes_one": int(cap.table_bytes),
           "prover_serialized_mixed_workspace_bytes": int(wsb), "build_s": build_s}
    if args.mixed_only:
        t_a = timed(torch, leg_a, args.reps, args.warmup)
        res.update({"A_one_call": stats(t_a), "A_proofs_per_s": count / (statistics.median(t_a) / 1e3)})
        return finish(args, res)
    ded = {}
    for m in MIX:
        if m == CAP:
            ded[m] = cap
            continue
        t0 = time.time()
        ded[m] = B.BatchVerifier(B.PublicKey.new(a, N * m), N, m, window_bits=args.window)
        build_s[str(m)] = time.time() - t0
    pos = {m: [j for j, (mm, _) in enumerate(order) if mm == m] for m in MIX}
    bufs = {}
    for m in MIX:
        idx = [order[j][1] for j in pos[m]]
        cnt, k = len(idx), (N * m).bit_length() - 1
        w = ded[m].prover_workspace_bytes(cnt)
        bufs[m] = (up(vals[m][idx].view(np.int64)), up(gams[m][idx].view(np.int64)),
                   torch.zeros((cnt, 3 + 2 * k, a.PW), dtype=torch.int64, device=dev),
                   torch.zeros((cnt, 3, 4), dtype=torch.int64, device=dev), torch.zeros((cnt, m, a.PW), dtype=torch.int64, device=dev),
                   torch.empty(w, dtype=torch.uint8, device=dev), w, cnt)

    def leg_b():
        for m in MIX:
            v, g, p, s, V, w, wb, cnt = bufs[m]
            ded[m].prove_batch_device(v.data_ptr(), g.data_ptr(), cnt, p.data_ptr(), s.data_ptr(), V.data_ptr(), w.data_ptr(), wb,
                                      stream(), transcript=True)

    lens = np.array([B.proof_bytes(a, N, m) for m in ms])
    starts = np.concatenate([[0], np.cumsum(lens)])
    cstarts = np.concatenate([[0], np.cumsum(np.array(ms) * B.compressed_bytes(a))])

    def leg_c():
        """-> (container bytes, commitment bytes) in caller order, through the host"""
        raw = np.empty(pbytes, dtype=np.uint8)
        cm = np.empty(cbytes, dtype=np.uint8)
        for m in MIX:
            v, g, p, s, V, w, wb, cnt = bufs[m]
            blobs = B.encode_proofs(a, N, m, p.cpu().numpy().view(np.uint64), s.cpu().numpy().view(np.uint64))
            comm = B.compress_points(a, V.cpu().numpy().view(np.uint64).reshape(-1, a.PW)).reshape(cnt, -1)
            sel = np.array(pos[m])
            raw[(starts[sel][:, None] + np.arange(blobs.shape[1])[None, :]).reshape(-1)] = blobs.reshape(-1)
            cm[(cstarts[sel][:, None] + np.arange(comm.shape[1])[None, :]).reshape(-1)] = comm.reshape(-1)
        return raw, cm

    for _ in range(args.warmup):
        leg_a()
        leg_b()
    torch.cuda.synchronize()
    t_a, t_b, t_c, same = [], [], [], True
    for _ in range(args.reps):
        t_a += timed(torch, leg_a, 1, 0)
        t_b += timed(torch, leg_b, 1, 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        raw, cm = leg_c()
        t_c.append((time.perf_counter() - t0) * 1e3)
        same &= bool(np.array_equal(d_raw.cpu().numpy(), raw) and np.array_equal(d_cm.cpu().numpy(), cm))
    # the block verifies where it lies
    d_ok = torch.full((count,), 7, dtype=torch.int32, device=dev)
    w2 = cap.serialized_mixed_workspace_bytes(ms)
    d_ws2 = torch.empty(w2, dtype=torch.uint8, device=dev)
    cap.verify_serialized_mixed_device(d_raw.data_ptr(), d_cm.data_ptr(), ms, d_ok.data_ptr(), d_ws2.data_ptr(), w2, stream(),
                                       transcript=True)
    med = {"A": statistics.median(t_a), "B": statistics.median(t_b), "C": statistics.median(t_c)}
    res.update({"A_one_call": stats(t_a), "B_five_dedicated_calls": stats(t_b), "C_host_encode_wall": stats(t_c),
                "A_bytes_equal_C_every_rep": same, "A_block_verifies": not bool(d_ok.cpu().numpy().any()),
                "A_minus_B_median_ms": med["A"] - med["B"], "B_spread_ms": max(t_b) - min(t_b),
                "A_within_B_spread": med["A"] - med["B"] <= max(t_b) - min(t_b),
                "ratio_A_over_B": med["A"] / med["B"], "ratio_A_over_B_plus_C": med["A"] / (med["B"] + med["C"]),
                "A_proofs_per_s": count / (med["A"] / 1e3),
                "table_bytes_dedicated_sum": int(sum(ded[m].table_bytes for m in MIX))})
    return finish(args, res)


def finish(args, res):
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
