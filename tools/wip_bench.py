#!/usr/bin/env python3
"""What the WIP seam costs: bpp_wip_verify_batch_device / bpp_wip_prove_batch_device against the range statement's own
calls on the SAME engine in the same process, the two alternated repetition by repetition (device events, after warm-up).

Per curve (BLS12-381, edwards25519), window_bits 13:
  a  verify, len 64, nv = 1, 4 096 proofs     against bpp_verifier_run at (64, 1): the two MulVecs have the same terms
  b  verify, len 1 024, nv = 16, 8 192 proofs  against bpp_verifier_run at (64, 16): the same number of terms (the
                                                reference normalises the m > 1 MulVec differently; the additions do not differ)
  c  prove, len 1 024, 2 048 proofs            against bpp_range_prove_batch_device at (64, 16)
The verify legs feed both calls the same records (made by the engine's range prover, a handful with a flipped s'), the seam
with the range statement's exponents (src/range/mod.rs:189-238, :405-477) as its statement; the verdict vectors are
compared.  The prove leg feeds the seam random a, b, y, gamma.  Prints one JSON object.
usage: python tools/wip_bench.py [--reps 20] [--warmup 3] [--window 13] [--curves bls12_381,ed25519] [--legs abc]
       [--scale 1.0] [--out profiles/wip_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "stdev_ms": statistics.stdev(ms) if len(ms) > 1 else 0.0, "reps": len(ms)}


def alternate(torch, fns, reps, warmup):
    """times the calls of `fns` alternately -> one list of milliseconds per call"""
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


def dev_scalars(torch, xs):
    import oracle as O
    return torch.from_numpy(O.scalars_to_wire(list(xs)).view(np.int64)).to("cuda:0")


def engine(B, cname, n, m, window):
    a = B.Arith.init(cname)
    return B.BatchVerifier(B.PublicKey.new(a, n * m), n, m, window_bits=window)


def range_batch(torch, bv, count, seed, tamper):
    """`count` range proofs made on the device -> (records (count, 3+2k+m, PW), scalars (count, 3, 4)) device tensors"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    PW, k, m = bv.arith.PW, bv.k, bv.m
    vals = torch.randint(0, 1 << 31, (count, m), generator=g, dtype=torch.int64).to("cuda:0")   # RangeProver::commit takes v as i32
    gams = torch.randint(0, 1 << 62, (count, m, 4), generator=g, dtype=torch.int64).to("cuda:0")
    gams[:, :, 3] &= (1 << 59) - 1    # below every curve's r
    d_p = torch.zeros((count, 3 + 2 * k, PW), dtype=torch.int64, device="cuda:0")
    d_s = torch.zeros((count, 3, 4), dtype=torch.int64, device="cuda:0")
    d_V = torch.zeros((count, m, PW), dtype=torch.int64, device="cuda:0")
    wsb = bv.prover_workspace_bytes(count)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    prove = lambda: bv.prove_batch_device(vals.data_ptr(), gams.data_ptr(), count, d_p.data_ptr(), d_s.data_ptr(),
                                          d_V.data_ptr(), d_ws.data_ptr(), wsb, stream)
    prove()
    torch.cuda.synchronize()
    rec = torch.cat([d_p, d_V], dim=1).contiguous()
    for j in range(tamper):
        d_s[(j * 997 + 13) % count, 1, 0] ^= 1
    return rec, d_s, prove


def verify_leg(torch, bv, count, window, reps, warmup, seed, tamper=8):
    import pyref as P
    import wip_cases as W
    n, m, k = bv.n, bv.m, bv.k
    r = P.CURVES[{0: "bls12_381", 1: "secp256k1", 2: "ed25519"}[bv.arith.curve]]["r"]
    rec, sc, _ = range_batch(torch, bv, count, seed, tamper)
    y, z = P.Transcript.yz(m)
    e = W.range_exponents(r, n, m, y, z)
    stm1 = dev_scalars(torch, list(e[0]) + list(e[1]) + [e[2]] + list(e[3]))
    d_stm = stm1.unsqueeze(0).repeat(count, 1, 1).contiguous()
    d_y = dev_scalars(torch, [y]).repeat(count, 1).contiguous()
    ok_r = torch.full((count,), 7, dtype=torch.int32, device="cuda:0")
    ok_w = torch.full((count,), 7, dtype=torch.int32, device="cuda:0")
    wsb_r, wsb_w = bv.workspace_bytes(count), bv.wip_verifier_workspace_bytes(count, m)
    ws_r = torch.empty(wsb_r, dtype=torch.uint8, device="cuda:0")
    ws_w = torch.empty(wsb_w, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    run = lambda: bv.run_device(rec.data_ptr(), sc.data_ptr(), count, ok_r.data_ptr(), ws_r.data_ptr(), wsb_r, stream)
    seam = lambda: bv.wip_verify_device(rec.data_ptr(), sc.data_ptr(), d_y.data_ptr(), d_stm.data_ptr(), m, count,
                                        ok_w.data_ptr(), ws_w.data_ptr(), wsb_w, stream)
    t_run, t_seam = alternate(torch, [run, seam], reps, warmup)
    a, b = ok_r.cpu().numpy(), ok_w.cpu().numpy()
    return {"len": n * m, "nv": m, "count": count, "range_run": stats(t_run), "wip_verify": stats(t_seam),
            "ratio_median": statistics.median(t_seam) / statistics.median(t_run),
            "verdicts_identical": bool((a == b).all()), "rejected": int(b.sum()),
            "extra_bytes_read_per_proof": (2 * n * m + 1 + m + 1) * 32}


def prove_leg(torch, bv, count, reps, warmup, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    ln, k = bv.n * bv.m, bv.k
    rnd = lambda *shape: torch.randint(-(1 << 63), (1 << 63) - 1, shape, generator=g, dtype=torch.int64).to("cuda:0")
    d_a, d_b, d_y, d_g = rnd(count, ln, 4), rnd(count, ln, 4), rnd(count, 4), rnd(count, 4)
    npts = bv.wip_points_per_proof(0)
    d_p = torch.zeros((count, npts, bv.arith.PW), dtype=torch.int64, device="cuda:0")
    d_s = torch.zeros((count, 3, 4), dtype=torch.int64, device="cuda:0")
    wsb = bv.wip_prover_workspace_bytes(count)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    seam = lambda: bv.wip_prove_device(d_a.data_ptr(), d_b.data_ptr(), d_y.data_ptr(), d_g.data_ptr(), count, 0,
                                       d_p.data_ptr(), d_s.data_ptr(), d_ws.data_ptr(), wsb, stream)
    _, _, rng_prove = range_batch(torch, bv, count, seed + 1, 0)
    t_rng, t_seam = alternate(torch, [rng_prove, seam], reps, warmup)
    return {"len": ln, "count": count, "range_prove": stats(t_rng), "wip_prove": stats(t_seam),
            "ratio_median": statistics.median(t_seam) / statistics.median(t_rng),
            "extra_bytes_read_per_proof": 2 * ln * 32, "virtual_proofs": {"range": 2 * k + 3 + bv.m, "wip": 2 * k + 2}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=int, default=13)
    ap.add_argument("--curves", default="bls12_381,ed25519")
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--scale", type=float, default=1.0, help="scales the proof counts (rehearsals)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("wip_bench needs a GPU: nothing here is measured on the CPU")
    import bulletproofsplus_amd as B
    cnt = lambda c: max(8, int(c * args.scale))
    res = {"window_bits": args.window, "device": torch.cuda.get_device_name(0), "curves": {}}
    for cname in args.curves.split(","):
        out = {}
        if "a" in args.legs:
            bv = engine(B, cname, 64, 1, args.window)
            out["a_verify_len64_nv1"] = verify_leg(torch, bv, cnt(4096), args.window, args.reps, args.warmup, 1)
            bv.close()
        if "b" in args.legs or "c" in args.legs:
            bv = engine(B, cname, 64, 16, args.window)
            if "b" in args.legs:
                out["b_verify_len1024_nv16"] = verify_leg(torch, bv, cnt(8192), args.window, args.reps, args.warmup, 2)
            if "c" in args.legs:
                out["c_prove_len1024"] = prove_leg(torch, bv, cnt(2048), args.reps, args.warmup, 3)
            bv.close()
        res["curves"][cname] = out
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
