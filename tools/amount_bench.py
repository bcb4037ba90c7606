#!/usr/bin/env python3
"""What BPP_PROVE_AMOUNT64 and the batched commitment kernel cost.  One process; every GPU step runs under a
time limit of its own (an alarm: a SLOW step ends the run there, with what was measured so far written out).  The alarm is
raised only when the interpreter has control again, so it does not bound a call that hangs inside the library or a
synchronise: run the whole tool under `timeout -k 10 <seconds>` as well.

  prove   bpp_range_prove_batch_mixed_device with the flag against the same call without it, the same values below 2^31,
          at (64, 16) x 2 048 and (64, 1) x 4 096 on BLS12-381: unflagged / flagged / unflagged alternated repetition by
          repetition.  The kernels are the same, so the expected ratio is 1; the margin is the spread of the two unflagged
          series in this process.
  commit  k_commit_batch at 2^12, 2^16, 2^20 commitments on each curve, (64, 1) engine at the bench window width, random
          64-bit amounts and random gammas, both modes: commitments/s, additions/s (count x mean non-zero digits of the
          inputs, recoded here as the kernel recodes them, over the kernel time from device events), and the share of the
          register-resident addition loop of tools/ubench.hip RUN IN THIS JOB (--ubench: the built binary; clocks differ
          between boxes, so a rate recorded elsewhere is not used).  For context the only batch route there was before:
          bpp_msm_batch with every length 2, host pointers, copies included.
  single  bpp_range_prove at (64, 1) on a repeated key with a hand-made untruncated commitment of 2^63 + 12345, cache on (the
          batch prover's second attempt, in amount mode) against cache off (the fold-based prover): wall time per call.  The
          outputs are identical by construction, so this timing is what tells the two paths apart.
usage: timeout -k 10 900 python tools/amount_bench.py [--reps 10] [--warmup 2] [--window 13] [--commit-window 16] [--ubench tools/ubench_bin]
       [--legs pcs] [--curves bls12_381,secp256k1,ed25519] [--scale 1.0] [--out profiles/amount_bench.json]"""
import argparse
import json
import os
import signal
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

Z2 = 0xd201000000010000 ** 2
FR_BITS = {"bls12_381": 255, "secp256k1": 256, "ed25519": 253}
UBENCH_KEY = {"bls12_381": "xyzz_madd_lazy_bls", "secp256k1": "xyzz_madd_lazy_secp", "ed25519": "xyzz_madd_lazy_ed"}


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


# ---- the digits of a scalar, as csrc/commit_walk.hpp cuts them (for the addition count only) ------------------------------
def uniform_nonzero(k, c, fr_bits):
    W = (fr_bits - 1) // c + 1
    v = k + sum(1 << (c * j + c - 1) for j in range(W - 1))
    half, n = 1 << (c - 1), 0
    for j in range(W - 1):
        n += ((v >> (c * j)) & ((1 << c) - 1)) != half
    return n + ((v >> (c * (W - 1))) != 0)


def glv_widths(c, fr_bits=255):
    """csrc/fixed_glv.hpp glv_layout: the widths of the W - 1 signed windows"""
    hmax = Z2 // 2 + 1
    W = ((fr_bits - 1) // c + 1) // 2
    ns, best = W - 1, None
    for S in range(ns, 128):
        q, rem = divmod(S, ns)
        if q + (1 if rem else 0) > 24:
            break
        wc = [q + (1 if j >= ns - rem else 0) for j in range(ns)]
        off, bias, entries = 0, 0, 0
        for cj in wc:
            bias |= 1 << (off + cj - 1)
            entries += 1 << (cj - 1)
            off += cj
        top = (hmax + bias) >> S
        if top == 0 or top >= 1 << 31:
            continue
        entries += top
        if best is None or entries < best[0]:
            best = (entries, wc, bias)
    return best[1], best[2]


def glv_nonzero(k, r, wc, bias):
    kk = r - k if k > (r - 1) // 2 else k
    k1, k2 = kk % Z2, kk // Z2
    if 2 * k1 > Z2:
        k1, k2 = Z2 - k1, k2 + 1
    n = 0
    for h in (k1, k2):
        v, off = h + bias, 0
        for cj in wc:
            n += ((v >> off) & ((1 << cj) - 1)) != (1 << (cj - 1))
            off += cj
        n += (v >> off) != 0
    return n


def mean_additions(cname, r, c, vs, gs, amount64):
    def i32(v):
        return (((v & 0xffffffff) ^ 0x80000000) - 0x80000000) % r
    ss = [v if amount64 else i32(v) for v in vs]
    if cname == "bls12_381":
        wc, bias = glv_widths(c)
        on_g = [glv_nonzero(s, r, wc, bias) for s in ss]
        on_h = [glv_nonzero(g, r, wc, bias) for g in gs]
    else:
        on_g = [uniform_nonzero(s, c, FR_BITS[cname]) for s in ss]
        on_h = [uniform_nonzero(g, c, FR_BITS[cname]) for g in gs]
    return statistics.mean(on_g), statistics.mean(on_h), max(on_g)


# ---- legs --------------------------------------------------------------------------------------------------------------
def prove_leg(torch, B, n, m, count, window, reps, warmup):
    a = B.Arith.init("bls12_381")
    bv = B.BatchVerifier(B.PublicKey.new(a, n * m), n, m, window_bits=window)
    g = torch.Generator(device="cpu").manual_seed(7 + m)
    vals = torch.randint(0, 1 << 31, (count, m), generator=g, dtype=torch.int64).to("cuda:0")
    gams = torch.randint(0, 1 << 62, (count, m, 4), generator=g, dtype=torch.int64).to("cuda:0")
    gams[:, :, 3] &= (1 << 59) - 1    # below r
    ms = [m] * count
    npts = bv.mixed_points(m) * count
    outs = [(torch.zeros((npts, a.PW), dtype=torch.int64, device="cuda:0"),
             torch.zeros((count, 3, 4), dtype=torch.int64, device="cuda:0")) for _ in range(2)]
    wsb = bv.prover_mixed_workspace_bytes(ms)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    def call(flag):
        d_p, d_s = outs[1 if flag else 0]
        return lambda: bv.prove_mixed_device(vals.data_ptr(), gams.data_ptr(), ms, d_p.data_ptr(), d_s.data_ptr(),
                                             d_ws.data_ptr(), wsb, stream, amount64=flag)
    t0, t1, t2 = alternate(torch, [call(False), call(True), call(False)], reps, warmup)
    same = bool(torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]))
    bv.close()
    m0, m1, m2 = (statistics.median(t) for t in (t0, t1, t2))
    base = (m0 + m2) / 2
    return {"n": n, "m": m, "count": count, "window_bits": window, "unflagged_a": stats(t0), "flagged": stats(t1),
            "unflagged_b": stats(t2), "ratio_flagged_over_unflagged": m1 / base,
            "spread_of_unflagged": abs(m0 - m2) / base, "outputs_identical_below_2_31": same,
            "proofs_per_s_flagged": count / (m1 * 1e-3)}


def commit_leg(torch, B, cname, window, counts, reps, warmup, loop_gops, msm_context):
    import pyref as P
    r = P.CURVES[cname]["r"]
    a = B.Arith.init(cname)
    pk = B.PublicKey.new(a, 64)
    bv = B.BatchVerifier(pk, 64, 1, window_bits=window)
    out = {"window_bits": window, "table_bytes": bv.table_bytes, "loop_gadd_per_s_same_job": loop_gops, "counts": {}}
    stream = torch.cuda.current_stream().cuda_stream
    for count in counts:
        rng = np.random.default_rng(1000 + count)
        vs = rng.integers(0, 1 << 64, size=count, dtype=np.uint64)
        gw = rng.integers(0, 1 << 64, size=(count, 4), dtype=np.uint64)
        gw[:, 3] &= np.uint64((1 << 59) - 1)    # below every curve's r
        d_v = torch.from_numpy(vs.view(np.int64)).to("cuda:0")
        d_g = torch.from_numpy(gw.view(np.int64)).to("cuda:0")
        d_o = torch.zeros((count, a.PW), dtype=torch.int64, device="cuda:0")
        sample = range(0, count, max(1, count // 4096))
        svs = [int(vs[i]) for i in sample]
        sgs = [sum(int(gw[i, t]) << (64 * t) for t in range(4)) for i in sample]
        row = {}
        for flag in (False, True):
            f = lambda: bv.commit_batch_device(d_v.data_ptr(), d_g.data_ptr(), count, d_o.data_ptr(), stream, amount64=flag)
            (t,) = alternate(torch, [f], reps, warmup)
            med = statistics.median(t)
            on_g, on_h, max_g = mean_additions(cname, r, window, svs, sgs, flag)
            adds = count * (on_g + on_h)
            e = {"kernel": stats(t), "commitments_per_s": count / (med * 1e-3), "mean_additions_on_g": on_g,
                 "mean_additions_on_h": on_h, "max_additions_on_g": max_g, "gadd_per_s": adds / (med * 1e-3) * 1e-9}
            if loop_gops:
                e["share_of_loop"] = e["gadd_per_s"] / loop_gops
            row["amount64" if flag else "i32"] = e
        if msm_context and count <= msm_context:
            # the batch route without the kernel: the untruncated point as count two-term MulVecs over (g, h), host pointers
            import time
            sc = np.zeros((2 * count, 4), dtype=np.uint64)
            sc[0::2, 0] = vs
            sc[1::2] = gw
            pts = np.tile(pk.gh, (count, 1))
            lens = np.full(count, 2, dtype=np.uint32)
            B.msm_batch(a, sc[:64], pts[:64], lens[:32])
            t0 = time.perf_counter()
            got = B.msm_batch(a, sc, pts, lens)
            dt = time.perf_counter() - t0
            row["msm_batch_len2_host"] = {"seconds": dt, "commitments_per_s": count / dt,
                                          "equals_kernel": bool(np.array_equal(got, d_o.cpu().numpy().view(np.uint64)))}
        out["counts"][str(count)] = row
    bv.close()
    return out


def single_leg(B, cname, reps):
    import time
    a = B.Arith.init(cname)
    pk = B.PublicKey.new(a, 64)
    v, gam = (1 << 63) + 12345, 987654321
    out = {}
    proofs = []
    for label, on in (("cache_on", True), ("cache_off", False)):
        a.set_verify_cache(on)
        ts = []
        for i in range(reps + 2):
            pr = B.RangeProver.new()
            pr.commit(pk, v, gam, amount64=True)
            t0 = time.perf_counter()
            pf = B.RangeProof.prove(pk, 64, pr)
            ts.append((time.perf_counter() - t0) * 1e3)
        pf.verify(pk, 64, pr.commitment_vec)
        proofs.append(pf.points_wire().tobytes() + pf.scalars_wire().tobytes())
        out[label] = stats(ts[2:])      # the first call sees the key, the second builds its engine
    a.set_verify_cache(True)
    out["outputs_identical"] = proofs[0] == proofs[1]
    out["speedup_median"] = out["cache_off"]["median_ms"] / out["cache_on"]["median_ms"]
    return out


def run_ubench(path):
    """the micro-benchmark binary as a child of its own, before this process opens the GPU -> its JSON (or None)"""
    if not path or not os.path.exists(path):
        return None
    p = subprocess.run([path], capture_output=True, text=True, timeout=240)
    if p.returncode != 0:
        raise SystemExit("ubench failed (%d): %s" % (p.returncode, p.stderr[-400:]))
    return json.loads(p.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=int, default=13)
    ap.add_argument("--commit-window", type=int, default=16)
    ap.add_argument("--ubench", default=os.path.join(ROOT, "tools", "ubench_bin"))
    ap.add_argument("--legs", default="pcs")
    ap.add_argument("--curves", default="bls12_381,secp256k1,ed25519")
    ap.add_argument("--scale", type=float, default=1.0, help="scales the counts (rehearsals)")
    ap.add_argument("--msm-context", type=int, default=1 << 16, help="largest count the bpp_msm_batch context leg runs at")
    ap.add_argument("--step-seconds", type=int, default=150)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ub = run_ubench(args.ubench) if "c" in args.legs else None
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("amount_bench needs a GPU: nothing here is measured on the CPU")
    import bulletproofsplus_amd as B
    cnt = lambda c: max(64, int(c * args.scale))
    res = {"device": torch.cuda.get_device_name(0), "ubench_same_job": ub is not None, "prove": {}, "commit": {}, "single": {}}

    def finish(code):
        text = json.dumps(res, indent=1)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        sys.exit(code)

    try:
        if "p" in args.legs:
            for (n, m, count) in ((64, 16, 2048), (64, 1, 4096)):
                res["prove"]["%dx%d_x%d" % (n, m, cnt(count))] = step(
                    args.step_seconds, lambda: prove_leg(torch, B, n, m, cnt(count), args.window, args.reps, args.warmup))
        if "c" in args.legs:
            for cname in args.curves.split(","):
                loop = ub[UBENCH_KEY[cname]]["Gops"] if ub and UBENCH_KEY[cname] in ub else None
                res["commit"][cname] = step(
                    args.step_seconds, lambda: commit_leg(torch, B, cname, args.commit_window, [cnt(1 << 12), cnt(1 << 16), cnt(1 << 20)],
                                                          args.reps, args.warmup, loop, args.msm_context))
        if "s" in args.legs:
            for cname in ("bls12_381", "secp256k1"):
                res["single"][cname] = step(args.step_seconds, lambda: single_leg(B, cname, args.reps))
    except StepTimeout:
        res["timed_out"] = True
        finish(3)
    finish(0)


if __name__ == "__main__":
    main()
