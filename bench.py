#!/usr/bin/env python3
"""bench.py -- aggregated range-proof verifies/sec on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--config c2|c3|c5] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps of the headline and prints the result line (with `roofline` and
`stage_ms` from the HIP events of those steps).  `--dump-outputs DIR` also writes what the last timed step computed:
DIR/verdicts.npy, the per-proof verdict words of the batch as float32 (0 = Ok), and DIR/mulvec_scalars.npy, the
verifier's MulVec scalars (reference MulVec order) of a seeded sample of up to 256 proofs, float64 of shape
(proofs, terms, 8): every 256-bit scalar as eight little-endian 32-bit words; DIR/mulvec_scalars_proofs.npy holds the
indices of the sampled proofs.  Ranks r > 0 add the suffix _rank<r>.  The inputs are the same from run to run for the
same arguments.  The tamper check, the side legs and the CPU
baseline listed below run only under `--full`, where the options of those legs apply.

A "step" is one pass of the hot path (RangeProof::verify for every proof of a resident batch:
verifier scalars -> fixed-generator MSM through the window tables -> proof-point MSM -> is_zero) over a
batch of synthetic proofs that is already in HBM when the timed region starts.

Configurations (BASELINE.json `configs`):
  c2 (default)  n=64, m=16 aggregated proofs, 8192 per GPU per step, BLS12-381 -- the metric's configuration
  c3            4096 independent n=64, m=1 proofs on one GPU
  c5            n=64, m=1, 8192 proofs per GPU (65 536 over 8 GPUs), mode-A all-reduce and mode-B all-gather legs

Multi-GPU: proofs are independent, so every rank verifies its own shard (weak scaling) and the only exchange
is one all-reduce of the failure count per step (the batch verdict, SURVEY.md 8e mode A).  With --gpus N > 1
and no WORLD_SIZE in the environment this script LAUNCHES the N ranks itself (fresh child processes, one per
GPU, before the parent has touched torch or the GPU); under `python -m torch.distributed.run` it is a rank.

Prints ONE JSON line on rank 0 (contract in the task statement), including
  "roofline"     : the dominant kernel (k_fixed_msm): duration from HIP events recorded on the launch stream
                   inside the timed region, algorithmic bytes per DESIGN.md; the kernel is integer-ALU bound, so
                   `alu` (mixed additions/s against the register-resident loop) is the meaningful ceiling;
  "cpu_baseline" : the CPU oracle (oracle/bpp_oracle.c, kind "port" -- the reference itself is Rust + the absent
                   mcl_rust and cannot be built) timed on bounded samples on this host: reference semantics
                   (naive MulVec) on one thread and on all cores, and a bucket-method (Pippenger) MulVec.
The oracle is used only for that leg.  Beside `value` (never as it) the line also carries separately timed legs:
"tamper_check" (exact verdict vector of the bench batch with K tampered proofs), "latency" (B = 1 / 16 / 256),
"prove" (batched device prover, device-resident), "serialized" (the same batch as proof containers + compressed
commitments: decode with subgroup check + verify; and as version-2 containers with uncompressed points),
"combined_check", "grouped_check" (per-proof verdicts from one weighted check per group of 32 proofs + an exact pass over
the groups that fail: all-valid and K-tampered batches), "c3" (4096 x (64,1)), "hard_distribution", "other_curves" (secp256k1, edwards25519: the metric's shape,
the C3 shape and one proof alone), "production" (hashed generators + Fiat-Shamir transcript + blinding from a key +
serialized input, with the stage split), "single_call" (RangeProof::prove / verify through the literal host-pointer API,
ms per call), "msm" (MulVec::calculate as a device-resident seam: N = 2^16..2^22 points on the three curves, with
`roofline` and `alu` per point), "sustained" (--sustained-steps) and, for world > 1, "comm_ms" (the exchange step).
Every leg ends with an untimed exact-verdict check on a tampered subset and carries a `roofline` block.
"""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec

CONFIGS = {
    # name: (n, m, proofs per GPU per step, window bits)
    "c2": (64, 16, 8192, 17),
    "c3": (64, 1, 4096, 16),
    "c5": (64, 1, 8192, 16),
}

# options of the checks and side legs beyond the headline, with their values under --full (a plain run runs none of them)
FULL_DEFAULTS = {"cpu_seconds": 5.0, "combined_steps": -1, "pipeline_streams": 2, "grouped_steps": 5, "other_curves_steps": 3,
                 "hard_steps": 4, "c3_steps": 5, "latency_steps": 5, "prove_steps": 2, "serialized_steps": 3, "sustained_steps": 0,
                 "production_steps": 3, "single_call_reps": 5, "msm_steps": 5, "tampered": 64}

# --dump-outputs stays under 64 MB: at most 4 Mi verdicts (float32) and the MulVec scalars of at most 256 proofs (float64)
# in 40 MB; larger outputs are written as a fixed, seeded sample
DUMP_VERDICTS = 4 << 20
DUMP_SCALAR_BYTES = 40 << 20


MSM_ORDER = {"bls12_381": 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
             "secp256k1": 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141,
             "ed25519": (1 << 252) + 27742317777372353535851937790883648493}


FR_BITS = {"bls12_381": 255, "secp256k1": 256, "ed25519": 253}


def loop_peaks(curve):
    """(G mixed additions/s of the register-resident loop, T v_mad_u64_u32 lane-ops/s, source file) recorded by
    tools/ubench.hip on this GPU model under profiles/ -- not measured in this run"""
    for cand in ("ubench_r03.json", "ubench_r02.json", "ubench_r01_final.json"):
        try:
            uj = json.load(open(os.path.join(ROOT, "profiles", cand)))
            key = {"bls12_381": "xyzz_madd_lazy_bls", "secp256k1": "xyzz_madd_lazy_secp", "ed25519": "xyzz_madd_lazy_ed"}.get(curve)
            if key is not None and key not in uj and key.replace("_lazy", "") not in uj:
                key = None
            if key is None:
                return None, uj["v_mad_u64_u32"]["Gops"] / 1e3, "profiles/" + cand
            if key not in uj:
                key = key.replace("_lazy", "")
            return uj[key]["Gops"], uj["v_mad_u64_u32"]["Gops"] / 1e3, "profiles/" + cand
        except Exception:
            continue
    return None, None, None


def verify_roofline(curve, n, m, batch, window_bits, kernel_ms, fp_bytes, kernel="k_fixed_msm", launches=None):
    """The roofline block of a verification leg, with the accounting of the headline: algorithmic bytes of one launch of
    the dominant kernel = batch x (2mn + 2) fixed terms x (affine point + scalar), against its mean duration
    (HIP events on the launch stream); `alu`: its table additions per second against the register-resident loop."""
    NF = 2 * n * m + 2
    term = 2 * fp_bytes + 32
    alg = batch * NF * term
    windows = (FR_BITS[curve] - 1) // window_bits + 1
    adds = batch * NF * windows
    ach = alg / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else 0.0
    rate = adds / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else 0.0
    add_peak, _, src = loop_peaks(curve)
    return {"bound": "hbm", "limiter": "alu", "kernel": kernel, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": ach / HBM_PEAK_GBS, "traffic": None, "algorithmic_bytes_per_launch": alg, "kernel_ms": kernel_ms,
            "launches_timed": launches,
            "alu": {"unit": "G mixed additions/s", "achieved": rate, "peak": add_peak,
                    "frac": (rate / add_peak) if add_peak else None, "additions_per_launch": adds, "peak_source": src}}


def synth_values(seed, m):
    """v_j = (0x9E3779B97F4A7C15 * (j+1+seed)) mod 2^31 (< 2^31 because of prover.rs:37), gamma_j = j+3+seed"""
    vals = [((0x9E3779B97F4A7C15 * (j + 1 + seed)) & 0xFFFFFFFFFFFFFFFF) % (1 << 31) for j in range(m)]
    gams = [j + 3 + seed for j in range(m)]
    return vals, gams


def host_cores():
    """CPU threads this process may really use: affinity mask, capped by a cgroup CPU quota when there is one."""
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                if q > 0:
                    per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                    n = min(n, max(1, q // per))
        except Exception:
            pass
    return max(1, n)


def cpu_baseline(n, m, curve_name, threads, min_seconds, pippenger_window=0):
    """Times oracle RangeProof::verify on `threads` threads for at least `min_seconds` of wall time.
    pippenger_window = 0: the reference's naive MulVec (mulvec.rs:20-33); else the bucket method."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import threading
    import oracle as O
    cid = O.CURVE_IDS[curve_name]
    pk = O.PublicKey(cid, n * m)
    gold = os.path.join(ROOT, "tests", "golden", "protocol_full_bls12_381.json")
    pts = sc = V = None
    if curve_name == "bls12_381" and (n, m) == (64, 16) and os.path.exists(gold):
        # verify cost does not depend on the proof (same MulVec length, full-width scalars): the golden (64,16)
        # proof serves every thread
        case = json.load(open(gold))[2]
        h = lambda p: (int(p[0], 16), int(p[1], 16))
        pts = O.points_to_wire(cid, [h(p) for p in case["points"]])
        V = O.points_to_wire(cid, [h(p) for p in case["V"]])
        sc = O.scalars_to_wire([int(case[k], 16) for k in ("r_prime", "s_prime", "d_prime")])
    else:
        vals, gams = synth_values(0, m)
        pts, sc, V = O.range_prove(pk, n, vals, gams)
    done = []
    stop = [False]

    def work():
        cnt = 0
        while True:
            rc = O.range_verify(pk, n, m, pts, sc, V, pippenger_window=pippenger_window)   # ctypes releases the GIL
            assert rc == 0
            cnt += 1
            if stop[0]:
                break
        done.append(cnt)

    t0 = time.perf_counter()
    ths = [threading.Thread(target=work) for _ in range(threads)]
    for t in ths:
        t.start()
    time.sleep(min_seconds)
    stop[0] = True
    for t in ths:
        t.join()
    dt = time.perf_counter() - t0
    return sum(done) / dt, dt, sum(done)


def free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(n):
    """--gpus N without a launcher: start N fresh rank processes (this parent never imports torch or touches the
    GPU), pass rank 0's stdout through, return the worst exit code."""
    port = os.environ.get("MASTER_PORT") or str(free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "MASTER_ADDR": "127.0.0.1",
                    "MASTER_PORT": port, "BPP_BENCH_LAUNCHED": "1"})
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    try:
        deadline = None
        while procs and any(p.poll() is None for p in procs):
            for p in procs:
                c = p.poll()
                if c not in (None, 0) and deadline is None:
                    deadline = time.time() + 20      # a rank died: give the others a moment, then stop them
                    rc = c
            if deadline is not None and time.time() > deadline:
                break
            time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=10)
            except Exception:
                p.kill()
    for p in procs:
        if p.returncode:
            rc = rc or p.returncode
    return rc


def dry_run(args):
    """Launcher / collective rehearsal WITHOUT a GPU (tests/test_bench_launcher.py, gloo on the CPU): the same
    rendezvous, barrier, failure-count all-reduce, partial all-gather and rank-0 JSON line as a real run, with the
    verification pass left out.  `value` is null: nothing is measured and nothing is verified here."""
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    ones = torch.ones(1, dtype=torch.int32)
    fail = torch.zeros(1, dtype=torch.int32)
    part = torch.full((160,), rank, dtype=torch.uint8)
    allp = torch.zeros(world * 160, dtype=torch.uint8)
    if world > 1:
        dist.barrier()
        for _ in range(args.steps):
            dist.all_reduce(fail, op=dist.ReduceOp.SUM)
            dist.all_gather_into_tensor(allp, part)
        dist.all_reduce(ones, op=dist.ReduceOp.SUM)
        dist.barrier()
    else:
        allp[:] = part
    seen = int(ones.item())
    assert allp.view(world, 160)[:, 0].tolist() == list(range(world))
    if rank == 0:
        n, m, bsz, _ = CONFIGS[args.config]
        print(json.dumps({"metric": "aggregated range-proof verifies/sec (n=%d,m=%d)" % (n, m), "value": None,
                          "unit": "verifies/s", "n_gpus": world, "ranks_seen": seen, "steps": args.steps,
                          "warmup": args.warmup, "dry_run": True, "config": {"workload": args.config}}))
    if world > 1:
        dist.destroy_process_group()


def timed(fn, steps, torch, dist, dev):
    """barrier + synchronize, `steps` calls, synchronize + barrier; returns max-over-ranks seconds
    (dev: where the reduced timing tensor lives -- the GPU under RCCL, the host in the gloo rehearsal)"""
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dist is not None:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS), help="BASELINE.json configuration (see module doc)")
    ap.add_argument("--batch", type=int, default=0, help="proofs per GPU per step (0 = the configuration's)")
    ap.add_argument("--distinct", type=int, default=0, help="distinct proofs per GPU; 0 = all of --batch distinct, else tiled")
    ap.add_argument("--curve", default="bls12_381", choices=["bls12_381", "secp256k1", "ed25519"])
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--m", type=int, default=0)
    ap.add_argument("--window", type=int, default=0,
                    help="window bits of the fixed-generator tables (c2: 17 = 204 GB for n=64, m=16 on BLS12-381)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the verdicts and a sample of the MulVec scalars of the last timed step to DIR (see module doc)")
    ap.add_argument("--full", action="store_true",
                    help="also run the tamper check, the side legs and the CPU baseline; the options below apply only with it")
    ap.add_argument("--cpu-seconds", type=float, default=None, help="wall seconds per CPU-baseline sample; 0 disables the CPU leg")
    ap.add_argument("--combined-steps", type=int, default=None,
                    help="extra (separately timed) steps of the combined batch check; -1 = same as --steps, 0 = skip")
    ap.add_argument("--pipeline-streams", type=int, default=None,
                    help="streams of the `pipelined` leg (the headline's passes alternating between them); < 2 = skip")
    ap.add_argument("--grouped-steps", type=int, default=None,
                    help="steps of the grouped check (per-proof verdicts from one weighted check per group); 0 = skip")
    ap.add_argument("--group", type=int, default=32, help="proofs per group of the grouped check (a power of two)")
    ap.add_argument("--other-curves-steps", type=int, default=None,
                    help="steps per extra leg on the other two instantiations of the same kernels (edwards25519 -- the curve "
                         "under Ristretto255, which BASELINE.json's configs[1] names -- and secp256k1); 0 = skip")
    ap.add_argument("--hard-steps", type=int, default=None,
                    help="steps of the 'hard distribution' leg (random generators, random full-width challenges; SURVEY 8d); 0 = skip")
    ap.add_argument("--c3-steps", type=int, default=None, help="steps of the C3 leg (4096 x (64,1)) of a c2 run; 0 = skip")
    ap.add_argument("--latency-steps", type=int, default=None, help="steps per small-batch latency point (B = 1, 16, 256); 0 = skip")
    ap.add_argument("--prove-steps", type=int, default=None, help="steps of the device-resident batched prover leg; 0 = skip")
    ap.add_argument("--serialized-steps", type=int, default=None,
                    help="steps of the serialized-input leg (containers + compressed commitments resident in HBM); 0 = skip")
    ap.add_argument("--sustained-steps", type=int, default=None,
                    help="extra back-to-back steps of the headline pass after the timed region (a 200-step run is kept in profiles/)")
    ap.add_argument("--production-steps", type=int, default=None,
                    help="steps of the production-path leg (hashed generators + transcript + serialized input); 0 = skip")
    ap.add_argument("--single-call-reps", type=int, default=None,
                    help="calls per point of the single_call leg (bpp_range_prove / bpp_range_verify, host pointers); 0 = skip")
    ap.add_argument("--msm-steps", type=int, default=None,
                    help="steps per point of the `msm` leg (device-resident general MulVec, N = 2^16 .. 2^22 on the three curves); 0 = skip")
    ap.add_argument("--msm-log2n", type=int, nargs="+", default=[16, 18, 20, 22])
    ap.add_argument("--tampered", type=int, default=None, help="tampered proofs of the untimed verdict check after the timed region")
    ap.add_argument("--dry-run", action="store_true", help="launcher/collective rehearsal without a GPU (see dry_run)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    for k, v in FULL_DEFAULTS.items():
        if getattr(args, k) is None:
            setattr(args, k, v if args.full else 0)
        elif not args.full:
            ap.error("--%s belongs to a check or side leg beyond the headline: add --full" % k.replace("_", "-"))

    # ---- launcher mode: must come before anything imports torch or touches the GPU ---------------------
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus))
    if args.dry_run:
        return dry_run(args)

    import numpy as np
    import torch
    import bulletproofsplus_amd as B

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # rehearsal knobs (not used by the driver): BPP_BENCH_BACKEND=gloo and BPP_BENCH_DEVICE=0 let two ranks share
    # the one GPU of a development box, to exercise the world > 1 control flow without RCCL
    backend = os.environ.get("BPP_BENCH_BACKEND", "nccl")
    if "BPP_BENCH_DEVICE" in os.environ:
        local_rank = int(os.environ["BPP_BENCH_DEVICE"])
    # BPP_BENCH_FORCE_DIST=1 (not used by the driver): go through the process group and its collectives even as the only
    # rank -- on a one-GPU box that is the way to have RCCL itself initialise and run the bench's all-reduce / all-gather
    force_dist = os.environ.get("BPP_BENCH_FORCE_DIST") == "1"
    if world > 1 or force_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group(backend="nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend=backend, rank=rank, world_size=world)
    else:
        dist = None
        torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    cn, cm, cb, cw = CONFIGS[args.config]
    n, m = args.n or cn, args.m or cm
    Bsz = args.batch or cb
    args.window = args.window or cw
    coll_dev = dev if backend == "nccl" else torch.device("cpu")     # gloo rehearsal: collectives on host tensors

    def allreduce_sum_i32(t):
        if backend == "nccl":
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        else:
            h = t.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM)
            t.copy_(h)

    # every rank is really there: sum of ones over the ranks
    ranks_seen = 1
    if dist is not None:
        one = torch.ones(1, dtype=torch.int32, device=dev)
        allreduce_sum_i32(one)
        ranks_seen = int(one.item())

    # ---- setup (untimed): generators, window tables, distinct proofs from the batched GPU prover -------
    a = B.Arith.init(args.curve, local_rank)
    pk = B.PublicKey.new(a, n * m)
    t1 = time.perf_counter()
    bv = None
    window = args.window
    window_requested = args.window
    while bv is None:
        try:
            bv = B.BatchVerifier(pk, n, m, window_bits=window)
        except B.BppError as e:
            # the c = 17 tables need 204 GB of free HBM (c = 16: 103 GB); fall back to narrower windows rather than
            # fail -- the width actually used is reported in config.window_bits
            if e.code != -5 or window <= 10:
                raise
            window -= 1
    args.window = window
    t_tables = time.perf_counter() - t1
    # every proof of the batch is distinct: values / blindings from a per-(rank, index) stream, proved by the
    # batched device prover (bit-identical to RangeProof::prove; tests/test_gpu_protocol.py)
    D = Bsz if args.distinct <= 0 else max(1, min(args.distinct, Bsz))
    t1 = time.perf_counter()
    vals, gams = [], []
    for d in range(D):
        v_, g_ = synth_values(rank * 1000003 + d * 17, m)
        vals.append(v_)
        gams.append(g_)
    pts_, scs, V_ = bv.prove_batch(vals, gams)
    t_prove = time.perf_counter() - t1
    recs = np.concatenate([pts_, V_], axis=1)
    if D < Bsz:
        idx = np.arange(Bsz) % D
        recs = recs[idx]
        scs = scs[idx]
    recs = np.ascontiguousarray(recs)
    scs = np.ascontiguousarray(scs)
    d_pts = torch.from_numpy(recs.view(np.int64)).to(dev)
    d_sc = torch.from_numpy(scs.view(np.int64)).to(dev)
    d_ok = torch.full((Bsz,), 7, dtype=torch.int32, device=dev)
    wsb = bv.workspace_bytes(Bsz)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    d_fail = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    # --dump-outputs: the pass also hands back its MulVec scalars (bpp_verifier_run's d_out_scalars), written there
    # instead of into the workspace -- the same kernels and the same work
    d_osc = torch.empty((Bsz, bv.msm_len, 4), dtype=torch.int64, device=dev) if args.dump_outputs else None

    comm_ev = []   # (before, after) events around the exchange step of every timed step (world > 1)

    def step(_i=0):
        bv.run_device(d_pts.data_ptr(), d_sc.data_ptr(), Bsz, d_ok.data_ptr(), d_ws.data_ptr(), wsb, stream,
                      d_out_scalars=d_osc.data_ptr() if d_osc is not None else 0)
        if dist is not None:
            # the one exchange step of the path: batch verdict = sum of per-proof failures over all ranks
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.sum(d_ok, dim=0, keepdim=True, out=d_fail)
            allreduce_sum_i32(d_fail)
            e1.record()
            comm_ev.append((e0, e1))

    for _ in range(args.warmup):
        step()
    d_ok.fill_(7)          # the verdicts read below are the timed steps' own, not the warm-up's
    torch.cuda.synchronize()
    bv.set_profiling(True)
    comm_ev.clear()
    dt = timed(step, args.steps, torch, dist, coll_dev)
    stage_ms, passes, bpp_ = bv.profile()
    bv.set_profiling(False)
    comm_ms = (sum(e0.elapsed_time(e1) for e0, e1 in comm_ev) / len(comm_ev)) if comm_ev else None
    ok = d_ok.cpu().numpy()
    if args.dump_outputs:
        # what a caller of the timed path receives from its last step: the verdict word of every proof (0 = Ok) and the
        # MulVec scalars of a seeded sample of the proofs, each 256-bit scalar as eight 32-bit words (exact in float64)
        os.makedirs(args.dump_outputs, exist_ok=True)
        sfx = "" if rank == 0 else "_rank%d" % rank
        out_v = ok.astype(np.float32)
        if out_v.size > DUMP_VERDICTS:
            out_v = out_v[np.sort(np.random.RandomState(0).choice(out_v.size, DUMP_VERDICTS, replace=False))]
        np.save(os.path.join(args.dump_outputs, "verdicts%s.npy" % sfx), out_v)
        S = max(1, min(256, Bsz, DUMP_SCALAR_BYTES // (bv.msm_len * 64)))
        pick = np.sort(np.random.RandomState(1).choice(Bsz, S, replace=False))
        words = d_osc[torch.from_numpy(pick).to(dev)].cpu().numpy().view(np.uint32)      # (S, msm_len, 8), little-endian
        np.save(os.path.join(args.dump_outputs, "mulvec_scalars%s.npy" % sfx), words.astype(np.float64))
        np.save(os.path.join(args.dump_outputs, "mulvec_scalars_proofs%s.npy" % sfx), pick.astype(np.float64))
        d_osc = None
        torch.cuda.empty_cache()
    # sustained: the same step many times back to back (clock drift / thermal check of the short timed region)
    sustained = None
    if args.sustained_steps > 0:
        sdt_ = timed(step, args.sustained_steps, torch, dist, coll_dev)
        sustained = {"steps": args.sustained_steps, "seconds": sdt_, "value": world * Bsz * args.sustained_steps / sdt_,
                     "ms_per_step": sdt_ / args.sustained_steps * 1e3}
    assert int(ok.sum()) == 0, "a valid proof failed to verify"
    if dist is not None:
        assert int(d_fail.item()) == 0

    # ---- untimed: the same batch geometry with K tampered proofs must give EXACTLY the expected verdict vector
    # (a kernel that wrote all-zero verdicts at this geometry would pass the assertion above)
    tamper = None
    if args.tampered > 0:
        K = min(args.tampered, Bsz)
        rs = np.random.RandomState(777 + rank)
        which = np.sort(rs.choice(Bsz, size=K, replace=False))
        sc_t = scs.copy()
        rec_t = recs.copy()
        kinds = []
        for j, i in enumerate(which):
            kind = j % 4
            kinds.append(kind)
            if kind < 3:
                sc_t[i, kind, 0] ^= np.uint64(1 << (j % 60))     # r', s' or delta' off by one bit
            else:
                src = (i + 1) % Bsz if D > 1 else i
                if np.array_equal(rec_t[src, 0], rec_t[i, 0]):
                    sc_t[i, 0, 1] ^= np.uint64(2)                  # identical proofs (tiled batch): tamper a scalar instead
                else:
                    rec_t[i, 0] = recs[src, 0]                     # the A of another proof
        d_pts_t = torch.from_numpy(np.ascontiguousarray(rec_t).view(np.int64)).to(dev)
        d_sc_t = torch.from_numpy(np.ascontiguousarray(sc_t).view(np.int64)).to(dev)
        d_ok.fill_(7)
        bv.run_device(d_pts_t.data_ptr(), d_sc_t.data_ptr(), Bsz, d_ok.data_ptr(), d_ws.data_ptr(), wsb, stream)
        torch.cuda.synchronize()
        got = d_ok.cpu().numpy()
        want = np.zeros(Bsz, dtype=got.dtype)
        want[which] = 1
        assert np.array_equal(got, want), "tampered batch: verdict vector differs from the expected one"
        tamper = {"batch": Bsz, "tampered": int(K), "verdicts_exact": True,
                  "kinds": "r' / s' / delta' bit flips and exchanged A points"}
        del d_pts_t, d_sc_t

    # ---- secondary, separately timed: the same passes alternating between two streams (two workspaces, two verdict
    # buffers).  Nothing in a pass depends on the previous one, so the last, partly idle round of one pass's k_fixed_msm
    # launch (and of the smaller launches around it) takes the next pass's scalar / proof-point kernels.  What a service
    # that keeps the verifier busy would do; the headline above stays one stream, where stage times add up to the step.
    pipelined = None
    if args.pipeline_streams > 1 and args.steps > 0:
        PS = args.pipeline_streams
        p_streams = [torch.cuda.Stream() for _ in range(PS)]
        p_ws = [torch.empty(wsb, dtype=torch.uint8, device=dev) for _ in range(PS)]
        p_ok = [torch.full((Bsz,), 7, dtype=torch.int32, device=dev) for _ in range(PS)]
        torch.cuda.synchronize()

        def pstep_pipe(i):
            q = i % PS
            bv.run_device(d_pts.data_ptr(), d_sc.data_ptr(), Bsz, p_ok[q].data_ptr(), p_ws[q].data_ptr(), wsb, p_streams[q].cuda_stream)
        for i in range(PS):
            pstep_pipe(i)
        pdt_pipe = timed(pstep_pipe, args.steps, torch, dist, coll_dev)
        assert all(int(o.sum().item()) == 0 for o in p_ok), "pipelined passes: a valid proof failed to verify"
        # untimed: the tampered batch through one of the lanes while the other runs the valid one: exact verdict vectors
        if tamper is not None:
            d_pts_t2 = torch.from_numpy(np.ascontiguousarray(rec_t).view(np.int64)).to(dev)
            d_sc_t2 = torch.from_numpy(np.ascontiguousarray(sc_t).view(np.int64)).to(dev)
            torch.cuda.synchronize()
            p_ok[0].fill_(7)
            p_ok[1].fill_(7)
            torch.cuda.synchronize()
            bv.run_device(d_pts.data_ptr(), d_sc.data_ptr(), Bsz, p_ok[0].data_ptr(), p_ws[0].data_ptr(), wsb, p_streams[0].cuda_stream)
            bv.run_device(d_pts_t2.data_ptr(), d_sc_t2.data_ptr(), Bsz, p_ok[1].data_ptr(), p_ws[1].data_ptr(), wsb, p_streams[1].cuda_stream)
            torch.cuda.synchronize()
            assert int(p_ok[0].sum().item()) == 0 and np.array_equal(p_ok[1].cpu().numpy(), want), \
                "pipelined passes: concurrent passes disturbed each other's verdicts"
            del d_pts_t2, d_sc_t2
        pipelined = {"value": world * Bsz * args.steps / pdt_pipe, "unit": "verifies/s", "streams": PS, "steps": args.steps,
                     "ms_per_step": pdt_pipe / args.steps * 1e3, "gain_over_one_stream": (dt / pdt_pipe) - 1.0,
                     "concurrent_verdicts_exact": tamper is not None,
                     "note": "the headline's passes alternating between %d streams with a workspace each: consecutive passes are "
                             "independent, so the partly idle last rounds of one pass's launches take the next pass's work; reported "
                             "beside `value`, whose single-stream stage times add up to its step" % PS}
        del p_ws, p_ok

    # ---- small-batch latency (B = 1 latency), same engine, same proofs ------------------
    latency = None
    if args.latency_steps > 0 and world == 1:
        latency = {}
        for Bl in (1, 16, 256):
            if Bl > Bsz:
                continue
            wl = bv.workspace_bytes(Bl)
            bv.run_device(d_pts.data_ptr(), d_sc.data_ptr(), Bl, d_ok.data_ptr(), d_ws.data_ptr(), max(wl, 1), stream)   # warm-up
            torch.cuda.synchronize()
            bv.set_profiling(True)
            dl = timed(lambda i: bv.run_device(d_pts.data_ptr(), d_sc.data_ptr(), Bl, d_ok.data_ptr(), d_ws.data_ptr(),
                                               max(wl, 1), stream), args.latency_steps, torch, None, dev)
            lst, _, _ = bv.profile()
            bv.set_profiling(False)
            assert int(d_ok[:Bl].sum().item()) == 0
            # the round trip a caller waits for -- enqueue, then synchronise, one pass at a time -- eagerly and as a replay
            # of the pass captured into a HIP graph by the library (bpp_verifier_graph_capture)
            def round_trip(fn):
                best = 1e9
                for _ in range(max(3, args.latency_steps)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    best = min(best, time.perf_counter() - t0)
                return best * 1e3
            rt = round_trip(lambda: bv.run_device(d_pts.data_ptr(), d_sc.data_ptr(), Bl, d_ok.data_ptr(), d_ws.data_ptr(),
                                                  max(wl, 1), stream))
            pg = bv.graph_capture(d_pts.data_ptr(), d_sc.data_ptr(), Bl, d_ok.data_ptr(), d_ws.data_ptr(), max(wl, 1))
            d_ok[:Bl].fill_(7)
            pg.launch(stream)
            torch.cuda.synchronize()
            assert int(d_ok[:Bl].sum().item()) == 0, "latency leg: the replayed graph gave other verdicts"
            rt_g = round_trip(lambda: pg.launch(stream))
            dg = timed(lambda i: pg.launch(stream), args.latency_steps, torch, None, dev)
            pg.close()
            latency["B=%d" % Bl] = {"ms": dl / args.latency_steps * 1e3, "verifies_per_s": Bl * args.latency_steps / dl,
                                    "stage_ms": {k: round(v, 4) for k, v in lst.items()},
                                    "graph_ms": dg / args.latency_steps * 1e3,
                                    "round_trip_ms": {"eager": rt, "graph_replay": rt_g,
                                                      "note": "wall clock of enqueue + synchronise of ONE pass (best of %d); `ms` "
                                                              "and `graph_ms` are passes enqueued back to back" % max(3, args.latency_steps)}}

    # ---- the batched prover with every buffer in HBM ---------------------------
    prove = None
    if args.prove_steps > 0:
        Pn = min(Bsz, 2048)
        pv = np.array(vals[:Pn] if D >= Pn else [vals[i % D] for i in range(Pn)], dtype=np.uint64)
        pg = np.zeros((Pn, m, 4), dtype=np.uint64)
        for i in range(Pn):
            pg[i, :, 0] = np.array(gams[i % D], dtype=np.uint64)
        d_pv = torch.from_numpy(pv.view(np.int64)).to(dev)
        d_pg = torch.from_numpy(pg.view(np.int64)).to(dev)
        kk = (n * m).bit_length() - 1
        d_po = torch.zeros((Pn, 3 + 2 * kk, a.PW), dtype=torch.int64, device=dev)
        d_ps = torch.zeros((Pn, 3, 4), dtype=torch.int64, device=dev)
        d_pV = torch.zeros((Pn, m, a.PW), dtype=torch.int64, device=dev)
        pwsb = bv.prover_workspace_bytes(Pn)
        d_pws = torch.empty(pwsb, dtype=torch.uint8, device=dev)

        def pstep(_i):
            bv.prove_batch_device(d_pv.data_ptr(), d_pg.data_ptr(), Pn, d_po.data_ptr(), d_ps.data_ptr(), d_pV.data_ptr(),
                                  d_pws.data_ptr(), pwsb, stream)

        pstep(0)
        pdt = timed(pstep, args.prove_steps, torch, dist, coll_dev)
        # the proofs the timed prover wrote are the ones the batch was built from (bit-exact), and they verify
        got_p = d_po.cpu().numpy().view(np.uint64)
        assert np.array_equal(got_p, pts_[np.arange(Pn) % D]), "device-resident prover output differs from prove_batch"
        # the same batch under the Fiat-Shamir transcript: every round's MulVecs wait for the previous round's hash
        def pstep_fs(_i):
            bv.prove_batch_device(d_pv.data_ptr(), d_pg.data_ptr(), Pn, d_po.data_ptr(), d_ps.data_ptr(), d_pV.data_ptr(),
                                  d_pws.data_ptr(), pwsb, stream, transcript=True)

        pstep_fs(0)
        pdt_fs = timed(pstep_fs, args.prove_steps, torch, dist, coll_dev)
        # untimed: the transcript-mode proofs the timed prover just wrote verify under the transcript, and a tampered
        # subset is rejected exactly
        recs_fs = torch.cat([d_po, d_pV], dim=1).contiguous()
        d_chf = torch.zeros((Pn, 3 + kk, 4), dtype=torch.int64, device=dev)
        bv.derive_challenges_device(recs_fs.data_ptr(), Pn, d_chf.data_ptr())
        sc_fs = d_ps.cpu().numpy().view(np.uint64).copy()
        Kp = min(32, Pn)
        which_p = np.sort(np.random.RandomState(31 + rank).choice(Pn, size=Kp, replace=False))
        for j, i in enumerate(which_p):
            sc_fs[i, j % 3, 0] ^= np.uint64(1 << (j % 50))
        d_scf = torch.from_numpy(sc_fs.view(np.int64)).to(dev)
        d_okp = torch.full((Pn,), 7, dtype=torch.int32, device=dev)
        wsp = bv.workspace_bytes(Pn)
        bv.run_device(recs_fs.data_ptr(), d_scf.data_ptr(), Pn, d_okp.data_ptr(), d_ws.data_ptr(), wsp, stream,
                      d_challenges=d_chf.data_ptr())
        torch.cuda.synchronize()
        want_p = np.zeros(Pn, dtype=np.int32)
        want_p[which_p] = 1
        assert np.array_equal(d_okp.cpu().numpy(), want_p), "prove leg: transcript-mode proofs / tampered subset: wrong verdicts"
        # MulVec terms of one RangeProof::prove: A-hat (mn + m + 3), L_t and R_t (2 n' + 2 each), wip.A (4),
        # wip.B (2), and 2 per commitment; the prover's launches run them over the fixed generators' tables
        mn_ = n * m
        prove_terms = (mn_ + m + 3) + 4 * (mn_ - 1) + 4 * kk + 6 + 2 * m
        palg = Pn * prove_terms * (2 * ((a.PW - 1) // 2 * 8) + 32)
        prove = {"value": world * Pn * args.prove_steps / pdt, "unit": "proofs/s", "batch": Pn, "steps": args.prove_steps,
                 "ms_per_step": pdt / args.prove_steps * 1e3,
                 "verified": {"transcript_proofs": int(Pn), "tampered": int(Kp), "verdicts_exact": True},
                 "roofline": {"bound": "hbm", "limiter": "alu", "kernel": "k_fixed_msm<..., 2> (+ k_pb_*): the whole step",
                              "algorithmic_bytes_per_launch": palg, "mulvec_terms_per_proof": prove_terms,
                              "kernel_ms": pdt / args.prove_steps * 1e3,
                              "achieved": palg / (pdt / args.prove_steps) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": palg / (pdt / args.prove_steps) / 1e9 / HBM_PEAK_GBS, "traffic": None},
                 "transcript_mode": {"value": world * Pn * args.prove_steps / pdt_fs, "unit": "proofs/s",
                                     "ms_per_step": pdt_fs / args.prove_steps * 1e3,
                                     "note": "challenges from the SHA-256 transcript on the device, round by round "
                                             "(engine mode; the reference hard-codes its challenges)"},
                 "note": "RangeProof::prove + the m commitments per proof, inputs and outputs resident in HBM; "
                         "bit-identical to the single-proof path (tests/test_gpu_protocol.py)"}
        del d_pws, d_po, d_ps, d_pV, recs_fs, d_chf, d_scf, d_okp

    # ---- secondary, separately timed: the same batch arriving SERIALIZED (the proof container + compressed
    # commitments, resident in HBM): header / encoding / subgroup / canonicity checks and decompression on the device,
    # then the same verification pass -- what a service that takes proofs off the wire runs per batch
    serialized = None
    if args.serialized_steps > 0:
        npp = pts_.shape[1]
        blobs = B.encode_proofs(a, n, m, pts_, scs[:D] if D < Bsz else scs)
        comm = B.compress_points(a, V_.reshape(-1, a.PW)).reshape(D, m, -1)
        if D < Bsz:
            blobs, comm = blobs[np.arange(Bsz) % D], comm[np.arange(Bsz) % D]
        d_bl = torch.from_numpy(np.ascontiguousarray(blobs)).to(dev)
        d_cm = torch.from_numpy(np.ascontiguousarray(comm)).to(dev)
        swsb = bv.serialized_workspace_bytes(Bsz)
        d_sws = torch.empty(swsb, dtype=torch.uint8, device=dev)
        d_sok = torch.full((Bsz,), 7, dtype=torch.int32, device=dev)

        def sstep(_i):
            bv.verify_serialized_device(d_bl.data_ptr(), d_cm.data_ptr(), Bsz, d_sok.data_ptr(), d_sws.data_ptr(), swsb,
                                        stream)

        sstep(0)
        bv.set_profiling(True)
        sdt = timed(sstep, args.serialized_steps, torch, dist, coll_dev)
        sst, _, _ = bv.profile()
        bv.set_profiling(False)
        assert int(d_sok.cpu().numpy().sum()) == 0, "a valid serialized proof failed to verify"
        # untimed: a batch with bad containers must give EXACTLY the expected status vector: 1 for a tampered r' / s' /
        # delta', 2 (FormatError) for a bad header byte, a non-canonical scalar, a malformed point encoding and -- on
        # BLS12-381 -- a curve point outside G1
        cbytes = comm.shape[2]
        hdr, pt0 = 12, 12
        sc0 = hdr + npp * cbytes
        bl_bad = np.ascontiguousarray(blobs).copy()
        Ks = min(60, Bsz)
        rs_s = np.random.RandomState(999 + rank)
        which_s = np.sort(rs_s.choice(Bsz, size=Ks, replace=False))
        want_s = np.zeros(Bsz, dtype=np.int64)
        order_s = MSM_ORDER[args.curve]
        torsion = None
        if args.curve == "bls12_381":
            import ctypes as _ct
            # (0, 2) has order 3 on y^2 = x^3 + 4: P + (0, 2) is on the curve and outside G1; its compressed form comes from
            # the engine's own group law (bpp_debug_point_op, op 0 = add)
            Tw = np.zeros(a.PW, dtype=np.uint64)
            Tw[(a.PW - 1) // 2] = 2
            mixed = np.zeros(a.PW, dtype=np.uint64)
            from bulletproofsplus_amd import _lib as _L
            assert _L.lib().bpp_debug_point_op(a.handle, 0, pts_[0, 1].ctypes.data_as(_ct.c_void_p), Tw.ctypes.data_as(_ct.c_void_p), 1,
                                               mixed.ctypes.data_as(_ct.c_void_p)) == 0
            torsion = B.compress_points(a, mixed[None])[0]
        for j, i in enumerate(which_s):
            kind = j % 5
            if kind == 0:
                bl_bad[i, sc0 + 32 * (j % 3)] ^= 1 << (j % 7)           # tampered scalar, still canonical with overwhelming probability
                val = int.from_bytes(bytes(bl_bad[i, sc0 + 32 * (j % 3):sc0 + 32 * (j % 3) + 32]), "little")
                want_s[i] = 1 if val < order_s else 2
            elif kind == 1:
                bl_bad[i, 4 + (j % 5)] ^= 0x40                            # version / curve / n / m / k byte of the header
                want_s[i] = 2
            elif kind == 2:
                v0 = int.from_bytes(bytes(bl_bad[i, sc0:sc0 + 32]), "little") + order_s
                if v0 < (1 << 256):
                    bl_bad[i, sc0:sc0 + 32] = np.frombuffer(v0.to_bytes(32, "little"), dtype=np.uint8)   # r' + r: non-canonical
                    want_s[i] = 2
            elif kind == 3:
                bl_bad[i, pt0 + cbytes * 3] ^= (0x80 if args.curve == "bls12_381" else 0x05)   # L_0: compression flag / prefix byte
                want_s[i] = 2
            else:
                bl_bad[i, sc0 + 64 + 1] ^= 2                              # delta'
                val = int.from_bytes(bytes(bl_bad[i, sc0 + 64:sc0 + 96]), "little")
                want_s[i] = 1 if val < order_s else 2
        if torsion is not None:       # proof 0's wip.A replaced by wip.A + T (T of order 3)
            bl_bad[0, pt0 + cbytes:pt0 + 2 * cbytes] = torsion
            want_s[0] = 2
        d_bl_bad = torch.from_numpy(bl_bad).to(dev)
        d_sok.fill_(7)
        bv.verify_serialized_device(d_bl_bad.data_ptr(), d_cm.data_ptr(), Bsz, d_sok.data_ptr(), d_sws.data_ptr(), swsb, stream)
        torch.cuda.synchronize()
        got_s = d_sok.cpu().numpy().astype(np.int64)
        assert np.array_equal(got_s, want_s), "serialized leg: status vector differs from the expected one at %s" % \
            np.nonzero(got_s != want_s)[0][:8].tolist()
        del d_bl_bad
        in_bytes = blobs.shape[1] + m * comm.shape[2]
        # PCIe-inclusive: the same call preceded by the host-to-device copy of the bytes (pinned host memory)
        h_bl, h_cm = torch.from_numpy(np.ascontiguousarray(blobs)).pin_memory(), torch.from_numpy(np.ascontiguousarray(comm)).pin_memory()

        def sstep_h(_i):
            d_bl.copy_(h_bl, non_blocking=True)
            d_cm.copy_(h_cm, non_blocking=True)
            sstep(_i)

        sstep_h(0)
        sdt_h = timed(sstep_h, args.serialized_steps, torch, dist, coll_dev)
        serialized = {"value": world * Bsz * args.serialized_steps / sdt, "unit": "verifies/s", "steps": args.serialized_steps,
                      "ms_per_step": sdt / args.serialized_steps * 1e3, "bytes_per_proof": int(in_bytes),
                      "points_decoded_per_proof": int(npp + m),
                      "from_pinned_host": {"value": world * Bsz * args.serialized_steps / sdt_h, "unit": "verifies/s",
                                           "ms_per_step": sdt_h / args.serialized_steps * 1e3},
                      "stage_ms": {k: round(v, 4) for k, v in sst.items()},
                      "decode_ms": sdt / args.serialized_steps * 1e3 - sum(sst.values()),
                      "status_check": {"bad_containers": int((want_s != 0).sum()), "statuses_exact": True,
                                       "kinds": "tampered scalars (1); header byte, non-canonical scalar, malformed point, point outside G1 (2)"},
                      "roofline": verify_roofline(args.curve, n, m, Bsz, args.window, sst["fixed_msm"], (a.PW - 1) // 2 * 8,
                                                  launches=args.serialized_steps),
                      "note": "input = the versioned proof container + compressed commitments (include/bpp_amd.h), already in "
                              "HBM; decode (square root, G1 subgroup check, canonicity) + verification; `from_pinned_host` "
                              "adds the PCIe copy of those bytes.  Engine data format: the reference never serializes"}
        # the same batch in container version 2 (uncompressed points: no square root at decode time, +48 bytes per point)
        if B.uncompressed_bytes(a):
            blobs2 = B.encode_proofs(a, n, m, pts_, scs[:D] if D < Bsz else scs, version=2)
            comm2 = B.uncompressed_points(a, V_.reshape(-1, a.PW)).reshape(D, m, -1)
            if D < Bsz:
                blobs2, comm2 = blobs2[np.arange(Bsz) % D], comm2[np.arange(Bsz) % D]
            d_bl2 = torch.from_numpy(np.ascontiguousarray(blobs2)).to(dev)
            d_cm2 = torch.from_numpy(np.ascontiguousarray(comm2)).to(dev)

            def sstep2(_i):
                bv.verify_serialized_device(d_bl2.data_ptr(), d_cm2.data_ptr(), Bsz, d_sok.data_ptr(), d_sws.data_ptr(), swsb,
                                            stream, uncompressed=True)
            sstep2(0)
            bv.set_profiling(True)
            sdt2 = timed(sstep2, args.serialized_steps, torch, dist, coll_dev)
            sst2, _, _ = bv.profile()
            bv.set_profiling(False)
            assert int(d_sok.cpu().numpy().sum()) == 0, "a valid version-2 container failed to verify"
            bl2_bad = np.ascontiguousarray(blobs2).copy()
            ub_ = comm2.shape[2]
            bl2_bad[1, 12 + ub_ - 1] ^= 1               # y of A: off the curve
            bl2_bad[2, 12 + (3 + 2 * ((n * m).bit_length() - 1)) * ub_ + 32] ^= 1   # s' off by one
            d_bl2b = torch.from_numpy(bl2_bad).to(dev)
            d_sok.fill_(7)
            bv.verify_serialized_device(d_bl2b.data_ptr(), d_cm2.data_ptr(), Bsz, d_sok.data_ptr(), d_sws.data_ptr(), swsb, stream,
                                        uncompressed=True)
            torch.cuda.synchronize()
            g2 = d_sok.cpu().numpy()
            assert g2[1] == 2 and g2[2] == 1 and int((g2 != 0).sum()) == 2, "version-2 containers: wrong statuses"
            serialized["uncompressed_container"] = {
                "value": world * Bsz * args.serialized_steps / sdt2, "unit": "verifies/s", "ms_per_step": sdt2 / args.serialized_steps * 1e3,
                "bytes_per_proof": int(blobs2.shape[1] + m * ub_), "decode_ms": sdt2 / args.serialized_steps * 1e3 - sum(sst2.values()),
                "note": "container version 2: uncompressed points (no square root at decode time)"}
            del d_bl2, d_cm2, d_bl2b
        del d_sws, d_bl, d_cm

    # ---- secondary, separately timed: the combined batch check (engine mode, not the reference's per-proof
    # semantics; see include/bpp_amd.h).  One weighted MulVec per rank, partials exchanged once per step.
    comb = None
    csteps = args.steps if args.combined_steps < 0 else args.combined_steps
    if csteps > 0:
        cwsb = bv.combined_workspace_bytes(Bsz)
        d_cws = torch.empty(cwsb, dtype=torch.uint8, device=dev)
        pbytes = bv.partial_bytes()
        d_part = torch.zeros(pbytes, dtype=torch.uint8, device=dev)
        d_all = torch.zeros(world * pbytes, dtype=torch.uint8, device=dev)
        d_cok = torch.full((1,), 7, dtype=torch.int32, device=dev)
        wkey = os.urandom(32)      # the weights' PRF key: fresh and secret per run

        def cstep(i):
            bv.run_combined_device(d_pts.data_ptr(), d_sc.data_ptr(), Bsz, wkey, rank * Bsz, d_part.data_ptr(),
                                   d_cok.data_ptr(), d_cws.data_ptr(), cwsb, stream)
            if dist is not None:
                # the single exchange: one partial (jacobian + validity word) per rank
                if backend == "nccl":
                    dist.all_gather_into_tensor(d_all, d_part)
                else:
                    h_all = torch.zeros(world * pbytes, dtype=torch.uint8)
                    dist.all_gather_into_tensor(h_all, d_part.cpu())
                    d_all.copy_(h_all)
                bv.sum_partials_device(d_all.data_ptr(), world, d_cok.data_ptr(), stream)

        cstep(0)
        cdt = timed(cstep, csteps, torch, dist, coll_dev)
        assert int(d_cok.item()) == 0, "combined check rejected an all-valid batch"
        # untimed: one tampered proof anywhere in the batch must flip the batch verdict
        sc_cb = scs.copy()
        sc_cb[(7 * Bsz) // 11, 2, 0] ^= np.uint64(1)
        d_sc_cb = torch.from_numpy(np.ascontiguousarray(sc_cb).view(np.int64)).to(dev)
        bv.run_combined_device(d_pts.data_ptr(), d_sc_cb.data_ptr(), Bsz, wkey, rank * Bsz, d_part.data_ptr(), d_cok.data_ptr(),
                               d_cws.data_ptr(), cwsb, stream)
        torch.cuda.synchronize()
        assert int(d_cok.item()) == 1, "combined check accepted a batch holding a tampered proof"
        del d_sc_cb
        calg = Bsz * bv.msm_len * (2 * ((a.PW - 1) // 2 * 8) + 32)     # every MulVec term of every proof enters the one combination
        comb = {"value": world * Bsz * csteps / cdt, "unit": "verifies/s", "steps": csteps, "ms_per_step": cdt / csteps * 1e3,
                "tamper_check": {"tampered": 1, "batch_verdict_flipped": True},
                "roofline": {"bound": "hbm", "limiter": "alu", "kernel": "k_comb_* + k_var_* + k_fixed_msm<..., 1>: the whole step",
                             "algorithmic_bytes_per_launch": calg, "kernel_ms": cdt / csteps * 1e3,
                             "achieved": calg / (cdt / csteps) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": calg / (cdt / csteps) / 1e9 / HBM_PEAK_GBS, "traffic": None},
                "note": "random-linear-combination batch check (weights = SHA-256 PRF of a fresh 256-bit key and the global "
                        "proof index): batch verdict only, NOT the reference's per-proof verdicts; reported beside `value`, "
                        "never as it"}
        del d_cws

    # ---- secondary, separately timed: the grouped check -- PER-PROOF verdicts from one weighted check per group of 32
    # neighbouring proofs, exact pass over the groups that fail (engine mode; include/bpp_amd.h "grouped check").
    # Three batches: all valid (the case it is for), K tampered proofs scattered (K groups re-verified), and the verdict
    # vector of the tampered batch compared with the exact path's expectation.
    grouped = None
    if args.grouped_steps > 0:
        GROUP = args.group
        gwsb = bv.grouped_workspace_bytes(Bsz, GROUP)
        d_gws = torch.empty(gwsb, dtype=torch.uint8, device=dev)
        d_gok = torch.full((Bsz,), 7, dtype=torch.int32, device=dev)
        gkey = os.urandom(32)
        gstats = [None]

        def gstep_on(dp, ds):
            def f(_i):
                gstats[0] = bv.run_grouped_device(dp.data_ptr(), ds.data_ptr(), Bsz, gkey, rank * Bsz, d_gok.data_ptr(),
                                                  d_gws.data_ptr(), gwsb, group=GROUP, stream=stream)
            return f
        gstep = gstep_on(d_pts, d_sc)
        gstep(0)
        gdt = timed(gstep, args.grouped_steps, torch, dist, coll_dev)
        assert int(d_gok.sum().item()) == 0 and gstats[0] == (0, 0), "grouped check: a valid batch did not come back all Ok"
        Kg = min(max(args.tampered, 1), Bsz)
        rsg = np.random.RandomState(4242 + rank)
        which_g = np.sort(rsg.choice(Bsz, size=Kg, replace=False))
        sc_g = scs.copy()
        for j, i in enumerate(which_g):
            sc_g[i, j % 3, 0] ^= np.uint64(1 << (j % 60))
        d_sc_g = torch.from_numpy(np.ascontiguousarray(sc_g).view(np.int64)).to(dev)
        gstep_t = gstep_on(d_pts, d_sc_g)
        gstep_t(0)
        gdt_t = timed(gstep_t, args.grouped_steps, torch, dist, coll_dev)
        got_g = d_gok.cpu().numpy()
        want_g = np.zeros(Bsz, dtype=got_g.dtype)
        want_g[which_g] = 1
        assert np.array_equal(got_g, want_g), "grouped check: verdict vector differs from the exact path's"
        groups_hit = len({int(i) // GROUP for i in which_g})
        assert gstats[0] == (groups_hit, groups_hit * GROUP), "grouped check: unexpected statistics %r" % (gstats[0],)
        # one host thread, two batches in flight (a stream, a workspace and a verdict buffer each): begin(A), begin(B),
        # finish(A), begin(A'), finish(B), ... -- the latency-bound parts of one batch hide behind the other
        g_pipe = None
        if args.pipeline_streams > 1 and pipelined is not None:
            PSg = 2
            # the streams of the `pipelined` leg again: ROCm maps streams onto a few hardware queues, and two streams created
            # at this point of the run shared one -- their passes ran strictly one after the other (measured: no gain at all)
            gp_streams = p_streams[:PSg]
            gp_ws = [torch.empty(gwsb, dtype=torch.uint8, device=dev) for _ in range(PSg)]
            gp_ok = [torch.full((Bsz,), 7, dtype=torch.int32, device=dev) for _ in range(PSg)]
            gp_in = [(d_pts, d_sc), (d_pts, d_sc_g)]     # lane 1 verifies the tampered batch all along
            torch.cuda.synchronize()

            def gp_begin(q):
                bv.grouped_begin_device(gp_in[q][0].data_ptr(), gp_in[q][1].data_ptr(), Bsz, gkey, rank * Bsz, gp_ok[q].data_ptr(),
                                        gp_ws[q].data_ptr(), gwsb, group=GROUP, stream=gp_streams[q].cuda_stream)

            def gp_finish(q):
                return bv.grouped_finish_device(gp_in[q][0].data_ptr(), gp_in[q][1].data_ptr(), Bsz, gp_ok[q].data_ptr(),
                                                gp_ws[q].data_ptr(), gwsb, group=GROUP, stream=gp_streams[q].cuda_stream)

            def run_pipe(steps, lanes_in):
                nonlocal gp_in
                gp_in = lanes_in
                gp_begin(0)
                for i in range(steps):
                    if i + 1 < steps:
                        gp_begin((i + 1) % PSg)
                    gp_finish(i % PSg)
            run_pipe(2, [(d_pts, d_sc), (d_pts, d_sc)])
            torch.cuda.synchronize()
            if dist is not None:
                dist.barrier()
            t0p = time.perf_counter()
            run_pipe(2 * args.grouped_steps, [(d_pts, d_sc), (d_pts, d_sc)])
            torch.cuda.synchronize()
            if dist is not None:
                dist.barrier()
            gpdt = time.perf_counter() - t0p
            assert all(int(o.sum().item()) == 0 for o in gp_ok), "grouped check, two in flight: a valid batch did not come back all Ok"
            run_pipe(2, [(d_pts, d_sc), (d_pts, d_sc_g)])    # a valid and the tampered batch in flight together
            torch.cuda.synchronize()
            assert int(gp_ok[0].sum().item()) == 0 and np.array_equal(gp_ok[1].cpu().numpy(), want_g), \
                "grouped check, two in flight: the batches disturbed each other's verdicts"
            g_pipe = {"value": world * Bsz * 2 * args.grouped_steps / gpdt, "unit": "verifies/s", "in_flight": PSg,
                      "ms_per_step": gpdt / (2 * args.grouped_steps) * 1e3, "concurrent_verdicts_exact": True,
                      "note": "bpp_verifier_grouped_begin / _finish from one host thread, two batches in flight"}
            del gp_ws, gp_ok
        galg = Bsz * bv.msm_len * (2 * ((a.PW - 1) // 2 * 8) + 32)
        gms = gdt / args.grouped_steps * 1e3
        grouped = {"value": world * Bsz * args.grouped_steps / gdt, "unit": "verifies/s", "steps": args.grouped_steps,
                   "ms_per_step": gms, "group": GROUP, "verdicts": "per proof", "two_in_flight": g_pipe,
                   "with_tampered": {"tampered": int(Kg), "groups_failed": groups_hit, "proofs_reverified": groups_hit * GROUP,
                                     "value": world * Bsz * args.grouped_steps / gdt_t, "unit": "verifies/s",
                                     "ms_per_step": gdt_t / args.grouped_steps * 1e3, "verdicts_exact": True},
                   "roofline": {"bound": "hbm", "limiter": "alu",
                                "kernel": "k_comb_* + k_var_* + k_fixed_msm<..., 0> over the groups: the whole step",
                                "algorithmic_bytes_per_launch": galg, "kernel_ms": gms,
                                "achieved": galg / gms / 1e6, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                "frac": galg / gms / 1e6 / HBM_PEAK_GBS, "traffic": None},
                   "note": "per-proof verdicts: one weighted check per group of %d neighbouring proofs (weights = SHA-256 PRF of a "
                           "fresh 256-bit key and the global proof index), then the exact per-proof path over the proofs of the "
                           "groups that failed; the verdict vector is the exact path's except with probability ~2^-128 per group.  "
                           "NOT the reference's deterministic per-proof check: reported beside `value`, never as it" % GROUP}
        del d_gws, d_sc_g, d_gok

    msm_len_main, table_bytes_main = bv.msm_len, bv.table_bytes

    # ---- secondary, separately timed: the "hard" distribution of SURVEY.md 8d.  Generators are random multiples
    # of g (SplitMix64 stream) instead of PublicKey::new's small multiples, and every proof is verified under its
    # own uniformly random full-width challenges instead of the reference's tiny constants.  Under random
    # challenges the proofs no longer verify -- the pass does exactly the same work either way (no early exit), so
    # this leg reports a rate, not verdicts; with the default challenges the same proofs are first checked to be Ok.
    hard = None
    if args.hard_steps > 0:
        order = {"bls12_381": 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
                 "secp256k1": 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141,
                 "ed25519": (1 << 252) + 27742317777372353535851937790883648493}[args.curve]
        state = [0xB0117E7 + 7919 * rank]

        def splitmix():
            state[0] = (state[0] + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
            z = state[0]
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
            return z ^ (z >> 31)

        def rand_scalar():
            return ((splitmix() << 192) | (splitmix() << 128) | (splitmix() << 64) | splitmix()) % order

        bv.close()                                  # the second set of tables needs the HBM of the first
        del d_ws
        torch.cuda.empty_cache()
        nf = 2 * n * m + 2
        ks = [rand_scalar() or 1 for _ in range(nf)]
        gens = a.scalar_mul(ks, np.repeat(pk.gh[:1], nf, axis=0))
        pk_h = B.PublicKey.from_points(a, gens[:2], gens[2:2 + n * m], gens[2 + n * m:])
        bv_h = B.BatchVerifier(pk_h, n, m, window_bits=args.window)
        pts_h, scs_h, V_h = bv_h.prove_batch(vals, gams)
        recs_h = np.ascontiguousarray(np.concatenate([pts_h, V_h], axis=1))
        if D < Bsz:
            recs_h = np.ascontiguousarray(recs_h[np.arange(Bsz) % D])
            scs_h = np.ascontiguousarray(scs_h[np.arange(Bsz) % D])
        d_pts_h = torch.from_numpy(recs_h.view(np.int64)).to(dev)
        d_sc_h = torch.from_numpy(np.ascontiguousarray(scs_h).view(np.int64)).to(dev)
        wsb_h = bv_h.workspace_bytes(Bsz)
        d_ws_h = torch.empty(wsb_h, dtype=torch.uint8, device=dev)
        kk = (n * m).bit_length() - 1
        ch = np.zeros((Bsz, 3 + kk, 4), dtype=np.uint64)
        rs = np.random.RandomState(12345 + rank)
        ch[:, :, :3] = rs.randint(0, 2**63, size=(Bsz, 3 + kk, 3), dtype=np.int64).astype(np.uint64) * np.uint64(2) + \
            rs.randint(0, 2, size=(Bsz, 3 + kk, 3)).astype(np.uint64)
        ch[:, :, 3] = rs.randint(1, 2**60, size=(Bsz, 3 + kk), dtype=np.int64).astype(np.uint64)   # < 2^252 <= every order
        d_ch = torch.from_numpy(ch.view(np.int64)).to(dev)
        bv_h.run_device(d_pts_h.data_ptr(), d_sc_h.data_ptr(), Bsz, d_ok.data_ptr(), d_ws_h.data_ptr(), wsb_h, stream)
        torch.cuda.synchronize()
        assert int(d_ok.sum().item()) == 0, "hard distribution: a valid proof failed under the default challenges"

        def hstep(_i):
            bv_h.run_device(d_pts_h.data_ptr(), d_sc_h.data_ptr(), Bsz, d_ok.data_ptr(), d_ws_h.data_ptr(), wsb_h, stream,
                            d_challenges=d_ch.data_ptr())

        hstep(0)
        bv_h.set_profiling(True)
        hdt = timed(hstep, args.hard_steps, torch, dist, coll_dev)
        hst, _, _ = bv_h.profile()
        bv_h.set_profiling(False)
        rejected = int((d_ok != 0).sum().item())
        hard = {"value": world * Bsz * args.hard_steps / hdt, "unit": "verifies/s", "steps": args.hard_steps,
                "ms_per_step": hdt / args.hard_steps * 1e3, "rejected_under_random_challenges": rejected,
                "stage_ms": {k: round(v, 4) for k, v in hst.items()},
                "roofline": verify_roofline(args.curve, n, m, Bsz, args.window, hst["fixed_msm"], (a.PW - 1) // 2 * 8,
                                            launches=args.hard_steps),
                "note": "random generators k_i*g (SplitMix64) and per-proof uniformly random full-width challenges (y, z, e, e_1..e_k) "
                        "through d_challenges: every MulVec scalar is full width; the proofs were made for the default "
                        "challenges, so they are rejected here -- the pass does the same work for valid and invalid proofs"}
        bv_h.close()
        del d_ws_h, d_pts_h, d_sc_h

    def release_main():
        nonlocal d_ws
        if bv.handle:
            bv.close()
        try:
            del d_ws
        except NameError:   # the hard-distribution leg has released it already
            pass
        torch.cuda.empty_cache()

    def side_leg(curve, n_, m_, batch, window_bits, steps, lat_steps=0):
        """the same pass on another curve / shape: fresh engine, GPU-proved distinct proofs, verdicts checked"""
        a_o = B.Arith.init(curve, local_rank)
        pk_o = B.PublicKey.new(a_o, n_ * m_)
        bv_o = B.BatchVerifier(pk_o, n_, m_, window_bits=window_bits)
        Do = min(batch, D)
        vo, go = [], []
        for d in range(Do):
            v_, g_ = synth_values(rank * 1000003 + d * 17, m_)
            vo.append(v_)
            go.append(g_)
        pts_o, scs_o, V_o = bv_o.prove_batch(vo, go)
        recs_o = np.ascontiguousarray(np.concatenate([pts_o, V_o], axis=1))
        scs_o = np.ascontiguousarray(scs_o)
        if Do < batch:
            recs_o = np.ascontiguousarray(recs_o[np.arange(batch) % Do])
            scs_o = np.ascontiguousarray(scs_o[np.arange(batch) % Do])
        d_pts_o = torch.from_numpy(recs_o.view(np.int64)).to(dev)
        d_sc_o = torch.from_numpy(scs_o.view(np.int64)).to(dev)
        d_ok_o = torch.full((batch,), 7, dtype=torch.int32, device=dev)
        wsb_o = bv_o.workspace_bytes(batch)
        d_ws_o = torch.empty(wsb_o, dtype=torch.uint8, device=dev)

        def ostep(_i):
            bv_o.run_device(d_pts_o.data_ptr(), d_sc_o.data_ptr(), batch, d_ok_o.data_ptr(), d_ws_o.data_ptr(), wsb_o, stream)

        ostep(0)
        torch.cuda.synchronize()
        assert int(d_ok_o.sum().item()) == 0, "%s (%d,%d): a valid proof failed to verify" % (curve, n_, m_)
        bv_o.set_profiling(True)
        odt = timed(ostep, steps, torch, dist, coll_dev)
        ost, _, obpp = bv_o.profile()
        bv_o.set_profiling(False)
        # untimed: the same geometry with a tampered subset must give EXACTLY the expected verdict vector (r', s', delta'
        # bit flips and, among distinct proofs, the A of another proof)
        Kt = min(64, batch)
        rs_t = np.random.RandomState(4242 + rank)
        which = np.sort(rs_t.choice(batch, size=Kt, replace=False))
        sc_bad = scs_o.copy()
        rec_bad = recs_o.copy()
        for j, i in enumerate(which):
            if j % 4 < 3 or Do < 2 or np.array_equal(recs_o[(i + 1) % batch, 0], recs_o[i, 0]):
                sc_bad[i, j % 3, 0] ^= np.uint64(1 << (j % 60))
            else:
                rec_bad[i, 0] = recs_o[(i + 1) % batch, 0]
        d_sc_b = torch.from_numpy(np.ascontiguousarray(sc_bad).view(np.int64)).to(dev)
        d_pts_b = torch.from_numpy(np.ascontiguousarray(rec_bad).view(np.int64)).to(dev)
        d_ok_o.fill_(7)
        bv_o.run_device(d_pts_b.data_ptr(), d_sc_b.data_ptr(), batch, d_ok_o.data_ptr(), d_ws_o.data_ptr(), wsb_o, stream)
        torch.cuda.synchronize()
        got = d_ok_o.cpu().numpy()
        want = np.zeros(batch, dtype=got.dtype)
        want[which] = 1
        assert np.array_equal(got, want), "%s (%d,%d): tampered batch: verdict vector differs from the expected one" % (curve, n_, m_)
        del d_pts_b
        res = {"value": world * batch * steps / odt, "unit": "verifies/s", "steps": steps, "ms_per_step": odt / steps * 1e3,
               "batch": batch, "window_bits": window_bits, "table_bytes": bv_o.table_bytes, "msm_terms_per_verify": bv_o.msm_len,
               "stage_ms": {k: round(v, 4) for k, v in ost.items()}, "blocks_per_proof": obpp,
               "tamper_check": {"tampered": int(Kt), "verdicts_exact": True},
               "roofline": verify_roofline(curve, n_, m_, batch, window_bits, ost["fixed_msm"], (a_o.PW - 1) // 2 * 8, launches=steps)}
        if lat_steps > 0:   # one proof alone on this engine (B = 1 latency)
            bv_o.run_device(d_pts_o.data_ptr(), d_sc_o.data_ptr(), 1, d_ok_o.data_ptr(), d_ws_o.data_ptr(), wsb_o, stream)
            torch.cuda.synchronize()
            bv_o.set_profiling(True)
            ldt = timed(lambda i: bv_o.run_device(d_pts_o.data_ptr(), d_sc_o.data_ptr(), 1, d_ok_o.data_ptr(), d_ws_o.data_ptr(),
                                                  wsb_o, stream), lat_steps, torch, None, dev)
            lst_o, _, _ = bv_o.profile()
            bv_o.set_profiling(False)
            assert int(d_ok_o[:1].item()) == 0
            res["latency_B=1"] = {"ms": ldt / lat_steps * 1e3, "stage_ms": {k: round(v, 4) for k, v in lst_o.items()}}
        bv_o.close()
        del d_ws_o, d_pts_o, d_sc_o, d_sc_b
        torch.cuda.empty_cache()
        return res

    # ---- secondary, separately timed: C3 of BASELINE.json (4096 independent n=64, m=1 proofs, one GPU) ----
    c3 = None
    if args.c3_steps > 0 and args.config == "c2" and args.curve == "bls12_381":
        release_main()
        c3 = side_leg("bls12_381", 64, 1, 4096, 16, args.c3_steps)
        c3["workload"] = "batch of 4096 independent n=64 m=1 proofs per GPU, per-proof verdicts"

    # ---- secondary, separately timed: the same shape on the other instantiations of the same kernel templates.
    # BASELINE.json's configs[1] names Ristretto; the reference has no such backend, so the
    # edwards25519 instantiation is parity-unpinned and can never be the headline; secp256k1 is the reference's
    # second in-tree backend.  Windows 17 / 16 (123 / 73 GB of tables).
    others = None
    if args.other_curves_steps > 0 and args.curve == "bls12_381":
        others = {}
        release_main()
        for oc in ("ed25519", "secp256k1"):
            # 253-bit group order: 15 windows at c = 17 against 16 at c = 16 (123 GB of tables); 256 bits need 16 either way
            others[oc] = side_leg(oc, n, m, Bsz, 17 if oc == "ed25519" else 16, args.other_curves_steps,
                                  lat_steps=args.latency_steps if world == 1 else 0)
            # BASELINE.json's C3 shape on this curve (4 096 x (64,1), c = 16)
            others[oc]["c3"] = side_leg(oc, 64, 1, 4096, 16, max(args.other_curves_steps, 3))
            others[oc]["parity"] = ("unpinned: not a reference backend; the prime-order subgroup of the curve under Ristretto255"
                                    if oc == "ed25519" else "the reference's second in-tree backend (not wired to its range proof)")

    # ---- secondary, separately timed: the PRODUCTION path -- what a maintainer adopting the README's API
    # (README.md:24-57: a transcript threaded through prove and verify) would run: generators hashed from a label
    # (bpp_pk_hashed; no known discrete logs), proofs made under the Fiat-Shamir transcript with blinding from a fresh
    # key, serialized, and then -- timed -- bytes in HBM -> decode -> derive challenges -> verify -> statuses.
    production = None
    if args.production_steps > 0 and args.curve == "bls12_381" and args.config == "c2":
        release_main()
        production = {}
        for (pn, pm, pbatch, pwin) in ((n, m, Bsz, args.window), (64, 1, 4096, 16)):
            a_p = B.Arith.init("bls12_381", local_rank)
            pk_p = B.PublicKey.hashed(a_p, pn * pm, b"bench production leg")
            bv_p = None
            while bv_p is None:
                try:
                    bv_p = B.BatchVerifier(pk_p, pn, pm, window_bits=pwin)
                except B.BppError as e:
                    if e.code != -5 or pwin <= 10:
                        raise
                    pwin -= 1
            kp = (pn * pm).bit_length() - 1
            Dp = min(pbatch, 2048)
            pv = np.array([synth_values(rank * 1000003 + d * 17, pm)[0] for d in range(Dp)], dtype=np.uint64)
            pg = np.zeros((Dp, pm, 4), dtype=np.uint64)
            for d in range(Dp):
                pg[d, :, 0] = np.array(synth_values(rank * 1000003 + d * 17, pm)[1], dtype=np.uint64)
            pts_p, scs_p, V_p = bv_p.prove_batch(pv, pg, transcript=True, blind_key=os.urandom(32), index_base=rank * pbatch)
            blobs_p = B.encode_proofs(a_p, pn, pm, pts_p, scs_p)
            comm_p = B.compress_points(a_p, V_p.reshape(-1, a_p.PW)).reshape(Dp, pm, -1)
            ix = np.arange(pbatch) % Dp
            blobs_p, comm_p = np.ascontiguousarray(blobs_p[ix]), np.ascontiguousarray(comm_p[ix])
            d_bl_p = torch.from_numpy(blobs_p).to(dev)
            d_cm_p = torch.from_numpy(comm_p).to(dev)
            swsb_p = bv_p.serialized_workspace_bytes(pbatch)
            d_sws_p = torch.empty(swsb_p, dtype=torch.uint8, device=dev)
            d_ok_p = torch.full((pbatch,), 7, dtype=torch.int32, device=dev)

            def prstep(_i):
                bv_p.verify_serialized_device(d_bl_p.data_ptr(), d_cm_p.data_ptr(), pbatch, d_ok_p.data_ptr(), d_sws_p.data_ptr(),
                                              swsb_p, stream, transcript=True)
            prstep(0)
            torch.cuda.synchronize()
            assert int(d_ok_p.cpu().numpy().sum()) == 0, "production leg: a valid proof failed to verify"
            bv_p.set_profiling(True)
            prdt = timed(prstep, args.production_steps, torch, dist, coll_dev)
            prst, _, _ = bv_p.profile()
            bv_p.set_profiling(False)
            # the derive step alone (SHA-256 transcript over the decoded records), on the records of the last pass
            recs_p = np.ascontiguousarray(np.concatenate([pts_p, V_p], axis=1)[ix])
            d_rec_p = torch.from_numpy(recs_p.view(np.int64)).to(dev)
            d_ch_p = torch.zeros((pbatch, 3 + kp, 4), dtype=torch.int64, device=dev)
            ddt = timed(lambda i: bv_p.derive_challenges_device(d_rec_p.data_ptr(), pbatch, d_ch_p.data_ptr()),
                        args.production_steps, torch, None, dev)
            # untimed: tampered subset -> exact statuses (1 for a flipped scalar bit; every proof point is bound by the transcript)
            Kq = min(48, pbatch)
            which_q = np.sort(np.random.RandomState(55 + rank).choice(pbatch, size=Kq, replace=False))
            bl_q = blobs_p.copy()
            cbp = comm_p.shape[2]
            sc0p = 12 + (3 + 2 * kp) * cbp
            want_q = np.zeros(pbatch, dtype=np.int64)
            for j, i in enumerate(which_q):
                if j % 2 == 0:
                    bl_q[i, sc0p + 32 * (j % 3) + 2] ^= 1 << (j % 8)
                    val = int.from_bytes(bytes(bl_q[i, sc0p + 32 * (j % 3):sc0p + 32 * (j % 3) + 32]), "little")
                    want_q[i] = 1 if val < MSM_ORDER["bls12_381"] else 2
                else:
                    bl_q[i, 5] ^= 1                                       # curve byte of the header
                    want_q[i] = 2
            d_bl_q = torch.from_numpy(bl_q).to(dev)
            d_ok_p.fill_(7)
            bv_p.verify_serialized_device(d_bl_q.data_ptr(), d_cm_p.data_ptr(), pbatch, d_ok_p.data_ptr(), d_sws_p.data_ptr(), swsb_p,
                                          stream, transcript=True)
            torch.cuda.synchronize()
            assert np.array_equal(d_ok_p.cpu().numpy().astype(np.int64), want_q), "production leg: status vector differs from the expected one"
            # the same bytes through the grouped check behind the decoder: the same status words, timed on the valid batch;
            # then the tampered batch must give the same exact status vector
            grouped_p = None
            if args.grouped_steps > 0:
                gwsb_p = bv_p.serialized_grouped_workspace_bytes(pbatch, args.group)
                d_gws_p = torch.empty(gwsb_p, dtype=torch.uint8, device=dev)
                gkey_p = os.urandom(32)
                gst_p = [None]

                def pgstep(_i, blobs=d_bl_p):
                    gst_p[0] = bv_p.verify_serialized_grouped_device(blobs.data_ptr(), d_cm_p.data_ptr(), pbatch, d_ok_p.data_ptr(),
                                                                     d_gws_p.data_ptr(), gwsb_p, gkey_p, rank * pbatch, args.group,
                                                                     stream, transcript=True)
                d_ok_p.fill_(7)
                pgstep(0)
                pgdt = timed(pgstep, args.production_steps, torch, dist, coll_dev)
                assert int(d_ok_p.cpu().numpy().sum()) == 0 and gst_p[0] == (0, 0), "production leg, grouped: a valid batch did not come back all Ok"
                d_ok_p.fill_(7)
                pgstep(0, d_bl_q)
                torch.cuda.synchronize()
                assert np.array_equal(d_ok_p.cpu().numpy().astype(np.int64), want_q), "production leg, grouped: status vector differs"
                # two host threads (the calls release the interpreter lock), each with its own stream, workspace and status
                # buffer: what two worker threads of a service sharing the verifier get
                two_threads = None
                if pipelined is not None:
                    import threading
                    t_ws = [d_gws_p, torch.empty(gwsb_p, dtype=torch.uint8, device=dev)]
                    t_ok = [torch.full((pbatch,), 7, dtype=torch.int32, device=dev) for _ in range(2)]
                    t_err = []
                    reps_t = max(2, args.production_steps)

                    def t_worker(q, reps):
                        try:
                            for _ in range(reps):
                                bv_p.verify_serialized_grouped_device(d_bl_p.data_ptr(), d_cm_p.data_ptr(), pbatch, t_ok[q].data_ptr(),
                                                                      t_ws[q].data_ptr(), gwsb_p, gkey_p, rank * pbatch, args.group,
                                                                      p_streams[q].cuda_stream, transcript=True)
                        except Exception as e:   # noqa: BLE001
                            t_err.append(repr(e))
                    torch.cuda.synchronize()
                    for q in range(2):
                        t_worker(q, 1)
                    torch.cuda.synchronize()
                    if dist is not None:
                        dist.barrier()
                    ths = [threading.Thread(target=t_worker, args=(q, reps_t)) for q in range(2)]
                    t0t = time.perf_counter()
                    for th in ths:
                        th.start()
                    for th in ths:
                        th.join()
                    torch.cuda.synchronize()
                    if dist is not None:
                        dist.barrier()
                    tdt = time.perf_counter() - t0t
                    assert not t_err and all(int(o.sum().item()) == 0 for o in t_ok), "production leg, two threads: %r" % (t_err,)
                    two_threads = {"value": world * pbatch * 2 * reps_t / tdt, "unit": "verifies/s",
                                   "ms_per_step": tdt / (2 * reps_t) * 1e3, "threads": 2}
                    del t_ws, t_ok
                grouped_p = {"value": world * pbatch * args.production_steps / pgdt, "unit": "verifies/s",
                             "ms_per_step": pgdt / args.production_steps * 1e3, "group": args.group, "two_threads": two_threads,
                             "status_check": {"tampered": int(Kq), "statuses_exact": True, "groups_failed": gst_p[0][0],
                                              "proofs_reverified": gst_p[0][1]},
                             "note": "bpp_range_verify_batch_serialized_grouped_device: decode + challenge derivation + one weighted "
                                     "check per group of proofs, exact pass over the groups that fail; per-proof statuses"}
                del d_gws_p
            ms_p = prdt / args.production_steps * 1e3
            derive_ms = ddt / args.production_steps * 1e3
            production["n=%d,m=%d" % (pn, pm)] = {
                "value": world * pbatch * args.production_steps / prdt, "unit": "verifies/s", "batch": pbatch, "steps": args.production_steps,
                "ms_per_step": ms_p, "window_bits": pwin, "table_bytes": bv_p.table_bytes,
                "bytes_per_proof": int(blobs_p.shape[1] + pm * cbp),
                "stage_ms": {"decode": round(ms_p - sum(prst.values()) - derive_ms, 4), "derive_challenges": round(derive_ms, 4),
                             **{k: round(v, 4) for k, v in prst.items()}},
                "status_check": {"tampered": int(Kq), "statuses_exact": True},
                "grouped": grouped_p,
                "roofline": verify_roofline("bls12_381", pn, pm, pbatch, pwin, prst["fixed_msm"], (a_p.PW - 1) // 2 * 8,
                                            launches=args.production_steps),
                "note": "generators hashed from a label (bpp_pk_hashed), proofs made under the SHA-256 transcript with blinding from a "
                        "fresh key, serialized containers + compressed commitments resident in HBM; timed: decode (square root, G1 "
                        "subgroup check) + challenge derivation + verification + status words; parity unpinned by the reference "
                        "(it has neither transcript nor serialization nor hashed generators)"}
            bv_p.close()
            del d_sws_p, d_bl_p, d_cm_p, d_rec_p, d_ch_p, d_bl_q
            torch.cuda.empty_cache()

    # ---- secondary: the LITERAL single-call API (src/range/mod.rs:31-78, src/main.rs:10-56): RangeProof::prove and
    # RangeProof::verify with host pointers and no verifier object, one proof per call.  ms per call, synchronous,
    # PCIe and allocations included.  verify: first call with a key = naive MulVec; second = builds that key's small
    # window tables; later calls = cached tables (include/bpp_amd.h, bpp_range_verify).
    single = None
    if args.single_call_reps > 0 and world == 1 and args.curve == "bls12_381":
        release_main()
        single = {}
        for (sn, sm) in ((32, 1), (64, 2), (64, 16)):
            a_s = B.Arith("bls12_381", local_rank)       # a context of its own: a clean verifier cache
            pk_s = B.PublicKey.new(a_s, sn * sm)
            pr_s = B.RangeProver.new()
            sv, sg = synth_values(5, sm)
            if (sn, sm) == (64, 2):
                sv, sg = [2, 5], [3, 7]                   # src/main.rs:20-27
            if sn < 64:
                sv = [v_ % (1 << sn) for v_ in sv]
            for v_, g_ in zip(sv, sg):
                pr_s.commit(pk_s, v_, g_)
            t0 = time.perf_counter()
            proof_s = B.RangeProof.prove(pk_s, sn, pr_s)
            t_first_prove = time.perf_counter() - t0
            tp = []
            for _ in range(args.single_call_reps):
                t0 = time.perf_counter()
                proof_s = B.RangeProof.prove(pk_s, sn, pr_s)
                tp.append(time.perf_counter() - t0)
            # verify in a context that has never seen this key (the prove calls above have already given a_s its cached
            # engine): first call = naive MulVec, second = builds the key's small tables, later = cached
            a_v = B.Arith("bls12_381", local_rank)
            pk_v = B.PublicKey.from_points(a_v, pk_s.gh, pk_s.G_vec, pk_s.H_vec)
            proof_v = B.RangeProof.from_wire(proof_s.points_wire(), proof_s.scalars_wire())
            tv = []
            for _ in range(2 + args.single_call_reps):
                t0 = time.perf_counter()
                proof_v.verify(pk_v, sn, pr_s.commitment_vec)     # raises on a wrong verdict
                tv.append(time.perf_counter() - t0)
            bad_s = B.RangeProof.from_wire(proof_s.points_wire(), proof_s.scalars_wire())
            bad_s.proof.r_prime = bad_s.proof.r_prime.copy()
            bad_s.proof.r_prime[0] ^= np.uint64(1)
            rejected = False
            try:
                bad_s.verify(pk_s, sn, pr_s.commitment_vec)
            except B.VerificationError:
                rejected = True
            assert rejected, "single_call: a tampered proof verified"
            a_s.set_verify_cache(False)
            tn = []
            for _ in range(args.single_call_reps):
                t0 = time.perf_counter()
                proof_s.verify(pk_s, sn, pr_s.commitment_vec)
                tn.append(time.perf_counter() - t0)
            single["n=%d,m=%d" % (sn, sm)] = {
                "prove_ms": min(tp) * 1e3, "prove_first_call_ms": t_first_prove * 1e3,
                "verify_first_call_ms": tv[0] * 1e3, "verify_second_call_builds_tables_ms": tv[1] * 1e3,
                "verify_cached_ms": min(tv[2:]) * 1e3, "verify_uncached_ms": min(tn) * 1e3,
                "msm_terms_per_verify": 2 * sn * sm + 2 * ((sn * sm).bit_length() - 1) + sm + 5}
        single["note"] = ("RangeProof::prove / RangeProof::verify through bpp_range_prove / bpp_range_verify: host pointers, one proof, "
                          "synchronous, wall clock of the call (best of %d); the tampered proof of each shape is rejected" % args.single_call_reps)

    # ---- secondary, separately timed: MulVec::calculate as a seam of its own at large N (bpp_msm_device) ---------
    # scalars and points resident in HBM, full-width scalars, distinct points k_i g (made on the GPU); every size is
    # checked against the known discrete logs: sum_i s_i (k_i g) == (sum_i s_i k_i) g.
    msm = None
    if args.msm_steps > 0 and args.curve == "bls12_381":
        release_main()
        msm = {"unit": "points/s", "steps": args.msm_steps,
               "workload": "one MulVec of N full-width scalars x N distinct points, all in HBM; result checked against the points' discrete logs",
               "curves": {}}
        try:
            uj = json.load(open(os.path.join(ROOT, "profiles", "ubench_r03.json")))
        except Exception:
            uj = {}
        def msm_traffic(curve_, lg_):
            # HBM bytes per launch of the dominant kernel (k_pip_chunks) from the recorded PMC profile, where one exists
            try:
                pj = json.load(open(os.path.join(ROOT, "profiles", "pmc_pip_chunks.json")))
                if pj.get("curve") == curve_ and pj.get("log2n") == lg_:
                    return pj.get("hbm_bytes_per_launch")
            except Exception:
                pass
            return None

        for mc in ("bls12_381", "secp256k1", "ed25519"):
            a_m = B.Arith.init(mc, local_rank)
            order = MSM_ORDER[mc]
            g_m = B.PublicKey.new(a_m, 0).gh[0]
            fpb = (a_m.PW - 1) // 2 * 8
            loop_peak = (uj.get({"bls12_381": "xyzz_madd_lazy_bls", "secp256k1": "xyzz_madd_lazy_secp", "ed25519": "xyzz_madd_lazy_ed"}.get(mc, "")) or {}).get("Gops")
            rows = []
            for lg in args.msm_log2n:
                N = 1 << lg
                rng = np.random.RandomState(1000 * rank + lg)
                ks = rng.randint(1, 2**62, size=N).astype(np.uint64)
                kw = np.zeros((N, 4), dtype=np.uint64)
                kw[:, 0] = ks
                pts_m = np.zeros((N, a_m.PW), dtype=np.uint64)
                for lo in range(0, N, 1 << 18):
                    hi = min(N, lo + (1 << 18))
                    pts_m[lo:hi] = a_m.scalar_mul(kw[lo:hi], np.broadcast_to(g_m, (hi - lo, a_m.PW)).copy())
                sc_m = rng.randint(0, 2**63 - 1, size=(N, 4)).astype(np.uint64) * np.uint64(2) + rng.randint(0, 2, size=(N, 4)).astype(np.uint64)
                sc_m[:, 3] >>= np.uint64(4)                   # < 2^252: below every curve's group order
                so = sc_m[:, 0].astype(object) + (sc_m[:, 1].astype(object) << 64) + (sc_m[:, 2].astype(object) << 128) + (sc_m[:, 3].astype(object) << 192)
                tot = int((so * ks.astype(object)).sum() % order)
                exp = a_m.scalar_mul(np.array([[(tot >> (64 * t)) & 0xFFFFFFFFFFFFFFFF for t in range(4)]], dtype=np.uint64), g_m[None])[0]
                d_sc_m = torch.from_numpy(sc_m.view(np.int64)).to(dev)
                d_pt_m = torch.from_numpy(pts_m.view(np.int64)).to(dev)
                d_out_m = torch.zeros(a_m.PW, dtype=torch.int64, device=dev)
                d_st_m = torch.full((1,), 7, dtype=torch.int32, device=dev)
                wsb_m = B.msm_workspace_bytes(a_m, N, 0)
                d_ws_m = torch.empty(wsb_m, dtype=torch.uint8, device=dev)

                def mstep(_i):
                    B.msm_device(a_m, d_sc_m.data_ptr(), d_pt_m.data_ptr(), N, d_out_m.data_ptr(), d_ws_m.data_ptr(), wsb_m,
                                 window_bits=0, d_status=d_st_m.data_ptr(), stream=stream)
                mstep(0)
                torch.cuda.synchronize()
                assert int(d_st_m.item()) == 0
                assert np.array_equal(d_out_m.cpu().numpy().view(np.uint64), exp), "msm leg: wrong sum at %s N=2^%d" % (mc, lg)
                B.msm_set_profiling(a_m, True)
                mdt = timed(mstep, args.msm_steps, torch, dist, coll_dev)
                mst, mpasses, mshape = B.msm_profile(a_m)
                B.msm_set_profiling(a_m, False)
                ms_call = mdt / args.msm_steps * 1e3
                alg = N * (2 * fpb + 32)                      # one affine point + one scalar per term
                madds = mshape["windows"] * mshape["items"]   # one bucket addition per (item, window); zero digits (2^-w of them) skipped
                kern_ms = sum(mst.values())
                add_rate = madds / (mst["chunks"] * 1e-3) / 1e9 if mst["chunks"] > 0 else 0.0
                rows.append({"log2n": lg, "ms": ms_call, "value": world * N / (ms_call * 1e-3),
                             "stage_ms": {k: round(v, 4) for k, v in mst.items()}, "shape": mshape,
                             "workspace_bytes": wsb_m,
                             "roofline": {"bound": "hbm", "limiter": "alu", "kernel": "k_pip_* (all stages of one call)",
                                          "algorithmic_bytes": alg, "kernel_ms": kern_ms,
                                          "achieved": alg / (kern_ms * 1e-3) / 1e9 if kern_ms > 0 else 0.0, "peak": HBM_PEAK_GBS,
                                          "unit": "GB/s", "frac": alg / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if kern_ms > 0 else 0.0,
                                          "traffic": msm_traffic(mc, lg),
                                          "alu": {"unit": "G mixed additions/s", "kernel": "k_pip_chunks", "additions": madds,
                                                  "additions_per_point": madds / N, "achieved": add_rate, "peak": loop_peak,
                                                  "frac": (add_rate / loop_peak) if loop_peak else None,
                                                  "whole_call_frac": (madds / (ms_call * 1e-3) / 1e9 / loop_peak) if loop_peak else None}}})
                del d_ws_m, d_sc_m, d_pt_m
                torch.cuda.empty_cache()
            msm["curves"][mc] = rows
        # the reference's MulVec::calculate is one scalar multiplication per term on one thread (mulvec.rs:28-31): the CPU
        # oracle's restatement of exactly that, timed on a bounded sample of the same kind of input
        if args.cpu_seconds > 0 and world == 1:
            try:
                sys.path.insert(0, os.path.join(ROOT, "oracle"))
                import oracle as O_
                a_c = B.Arith.init("bls12_381", local_rank)
                g_c = B.PublicKey.new(a_c, 0).gh[0]
                ns = 512
                rng = np.random.RandomState(7)
                kw = np.zeros((ns, 4), dtype=np.uint64)
                kw[:, 0] = rng.randint(1, 2**62, size=ns).astype(np.uint64)
                pts_c = a_c.scalar_mul(kw, np.broadcast_to(g_c, (ns, a_c.PW)).copy())
                sc_c = rng.randint(0, 2**63 - 1, size=(ns, 4)).astype(np.uint64)
                sc_c[:, 3] >>= np.uint64(4)
                t0 = time.perf_counter()
                res_c = O_.msm(0, sc_c, pts_c)
                dt_c = time.perf_counter() - t0
                d_o = torch.zeros(a_c.PW, dtype=torch.int64, device=dev)
                wsb_c = B.msm_workspace_bytes(a_c, ns, 0)
                d_w = torch.empty(wsb_c, dtype=torch.uint8, device=dev)
                d_sc_c = torch.from_numpy(sc_c.view(np.int64)).to(dev)
                d_pt_c = torch.from_numpy(pts_c.view(np.int64)).to(dev)
                B.msm_device(a_c, d_sc_c.data_ptr(), d_pt_c.data_ptr(), ns, d_o.data_ptr(), d_w.data_ptr(), wsb_c, stream=stream)
                torch.cuda.synchronize()
                assert np.array_equal(d_o.cpu().numpy().view(np.uint64), res_c), "msm leg: device MulVec differs from the oracle's on the CPU sample"
                msm["cpu_baseline"] = {"value": ns / dt_c, "unit": "points/s", "cores": 1, "kind": "port",
                                       "sample": "one naive MulVec of %d full-width terms on BLS12-381 by the CPU oracle (reference semantics, "
                                                 "mulvec.rs:20-33; the reference is single-threaded), %.2f s wall; the device result of the same "
                                                 "input is bit-identical" % (ns, dt_c)}
            except Exception as e:   # the oracle is optional test infrastructure: the leg stands without it
                msm["cpu_baseline"] = {"error": str(e)[:200]}
        msm["value"] = msm["curves"]["bls12_381"][-1]["value"]
        msm["note"] = ("value = the largest BLS12-381 point; roofline.achieved = N x (affine point + scalar) bytes / the summed stage "
                       "time of one call (HIP events on the launch stream) -- integer-ALU bound like the verifier; alu = bucket additions "
                       "per second of k_pip_chunks against the register-resident loop of the same addition (profiles/ubench_r03.json)")

    if rank == 0:
        N_msm = msm_len_main
        NF = 2 * n * m + 2
        fp_bytes = (a.PW - 1) // 2 * 8
        term_bytes = 2 * fp_bytes + 32                      # affine point + scalar
        value = world * Bsz * args.steps / dt
        dom_ms = stage_ms["fixed_msm"]
        alg_bytes = Bsz * NF * term_bytes                   # algorithmic bytes of one k_fixed_msm launch
        achieved = alg_bytes / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0
        # the ALU-side view of the same kernel: mixed additions per second against the rate of a register-resident
        # loop of the same addition (tools/ubench.hip on this GPU model, recorded in profiles/)
        fr_bits = {"bls12_381": 255, "secp256k1": 256, "ed25519": 253}[args.curve]
        windows = (fr_bits - 1) // args.window + 1
        adds = Bsz * NF * windows
        add_rate = adds / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0
        add_peak = mad_peak = None
        peak_file = None
        for cand in ("ubench_r03.json", "ubench_r02.json", "ubench_r01_final.json"):
            try:
                uj = json.load(open(os.path.join(ROOT, "profiles", cand)))
                key = {"bls12_381": "xyzz_madd_lazy_bls", "secp256k1": "xyzz_madd_lazy_secp", "ed25519": "xyzz_madd_lazy_ed"}[args.curve]
                if key not in uj:
                    key = key.replace("_lazy", "")
                add_peak = uj[key]["Gops"]
                mad_peak = uj["v_mad_u64_u32"]["Gops"] / 1e3          # T lane-ops/s, issue-rate micro-benchmark
                peak_file = "profiles/" + cand
                break
            except Exception:
                add_peak = mad_peak = None
        # multiplier work of one XYZZ mixed addition (8M + 2S, Y3 with one shared reduction) in v_mad_u64_u32 lane-ops:
        # NL^2 per product, NL(NL+1)/2 per squaring, NL^2 + NL per Montgomery reduction (9 of them); NL = 13 / 9 limbs
        nl = 13 if args.curve == "bls12_381" else 9
        mads_per_add = 8 * nl * nl + 2 * (nl * (nl + 1) // 2) + 9 * (nl * nl + nl)
        mad_rate = add_rate * mads_per_add / 1e3                   # T v_mad_u64_u32 lane-ops/s
        traffic = traffic_src = None
        pmc = os.path.join(ROOT, "profiles", "pmc_fixed_msm.json")
        if os.path.exists(pmc):
            try:
                pj = json.load(open(pmc))
                if pj.get("batch") == Bsz and pj.get("window") == args.window and pj.get("curve") == args.curve:
                    traffic = pj.get("hbm_bytes_per_launch")
                    traffic_src = "recorded PMC profile profiles/pmc_fixed_msm.json (FETCH_SIZE + WRITE_SIZE, separate passes), not measured in this run"
            except Exception:
                traffic = None
        out = {
            "metric": "aggregated range-proof verifies/sec (n=%d,m=%d)" % (n, m),
            "value": value, "unit": "verifies/s", "n_gpus": world, "ranks_seen": ranks_seen, "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u32 (30-bit limbs of a %d-bit prime field, v_mad_u64_u32)" % (381 if args.curve == "bls12_381" else 256),
            "data": "synthetic: %d distinct GPU-proved proofs per GPU in a batch of %d; reference constants as transcript" % (D, Bsz),
            "config": {"workload": "%s: n=%d m=%d range-proof verify, %s, batch %d per GPU, per-proof verdicts" % (args.config, n, m, args.curve, Bsz),
                       "curve": args.curve, "msm_terms_per_verify": N_msm, "window_bits": args.window,
                       "window_bits_requested": window_requested,
                       "window_narrowed_for_lack_of_hbm": args.window != window_requested,
                       "table_bytes": table_bytes_main,
                       "table_frac_of_hbm": table_bytes_main / float(torch.cuda.get_device_properties(dev).total_memory),
                       "parallelism": "proof-sharded x%d" % world,
                       "launcher": "bench.py spawned the ranks" if os.environ.get("BPP_BENCH_LAUNCHED") else
                                   ("external launcher" if world > 1 else "single process"),
                       "backend": backend if dist is not None else None},
            "roofline": {"bound": "hbm", "limiter": "alu", "kernel": "k_fixed_msm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                         "algorithmic_bytes_per_launch": alg_bytes, "kernel_ms": dom_ms, "launches_timed": passes,
                         "blocks_per_proof": bpp_,
                         "alu": {"unit": "G mixed additions/s", "achieved": add_rate, "peak": add_peak,
                                 "frac": (add_rate / add_peak) if add_peak else None,
                                 "additions_per_launch": adds,
                                 "field_products_per_s": add_rate * 10e9,
                                 "v_mad_u64_u32": {"unit": "T lane-ops/s", "achieved": mad_rate, "peak": mad_peak,
                                                   "frac": (mad_rate / mad_peak) if mad_peak else None,
                                                   "per_addition": mads_per_add},
                                 "peak_source": "register-resident XYZZ mixed-addition loop and v_mad_u64_u32 issue rate, tools/ubench.hip, "
                                                "recorded in %s (not measured in this run)" % peak_file},
                         "note": "`bound` names the roofline `achieved`/`peak`/`frac` are measured against, as the contract asks (HBM, algorithmic "
                                 "bytes); the kernel itself is integer-ALU bound (DESIGN.md section 4): `limiter`, and `alu` is the "
                                 "ceiling that binds"},
            "stage_ms": stage_ms,
            "tamper_check": tamper,
            "pipelined": pipelined,
            "latency": latency,
            "prove": prove,
            "serialized": serialized,
            "combined_check": comb,
            "grouped_check": grouped,
            "c3": c3,
            "hard_distribution": hard,
            "other_curves": others,
            "msm": msm,
            "production": production,
            "single_call": single,
            "sustained": sustained,
            "comm_ms": comm_ms,
            "setup_s": {"prove_batch_%d" % D: t_prove, "tables": t_tables},
        }
        if args.cpu_seconds > 0 and world == 1 and args.curve != "ed25519":   # the C oracle has no Edwards backend
            cores = host_cores()
            v1, d1, c1 = cpu_baseline(n, m, args.curve, 1, args.cpu_seconds)
            vN, dN, cN = cpu_baseline(n, m, args.curve, cores, args.cpu_seconds)
            vp, dp, cp = cpu_baseline(n, m, args.curve, cores, args.cpu_seconds, pippenger_window=8)
            out["cpu_baseline"] = {
                "value": vN, "unit": "verifies/s", "cores": cores, "kind": "port",
                "sample": "%d x RangeProof::verify (n=%d,m=%d) of the CPU oracle on %d threads, naive MulVec as the reference "
                          "(mulvec.rs:20-33), %.1f s wall" % (cN, n, m, cores, dN),
                "single_thread": {"value": v1, "cores": 1, "sample": "%d verifies, %.1f s wall (the reference is single-threaded)" % (c1, d1)},
                "pippenger": {"value": vp, "cores": cores,
                              "sample": "%d verifies, %.1f s wall; same oracle with a bucket-method MulVec (8-bit windows) -- what a tuned "
                                        "CPU library would run, NOT the reference's algorithm" % (cp, dp)},
                "note": "mcl's hand-written asm + GLV would beat this restatement per scalar multiplication: a lower bound on the reference's speed"}
        else:
            out["cpu_baseline"] = None
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
