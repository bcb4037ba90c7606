"""-m gpu: a plain `bench.py` run (no --full) in a small shape: the result line of the headline alone, `--steps` timed
steps, and --dump-outputs writing the verdicts and sampled MulVec scalars of the last timed step: the same in two runs
with the same arguments, and the scalars equal to what the verifier hands back for those proofs through the API."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c3", "--batch", "256", "--window", "10",
           "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)]
    out = subprocess.check_output(cmd, timeout=600)
    lines = [l for l in out.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_and_dump_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    line = _plain_run(tmp_path / "a")
    assert line["metric"] == "aggregated range-proof verifies/sec (n=64,m=1)" and line["unit"] == "verifies/s"
    assert line["higher_is_better"] is True and line["value"] > 0 and line["steps"] == 3
    assert line["ms_per_step"] == pytest.approx(256 * 1e3 / line["value"], rel=1e-9)
    assert line["tamper_check"] is None and line["cpu_baseline"] is None and line["combined_check"] is None
    v = np.load(tmp_path / "a" / "verdicts.npy")
    assert v.dtype == np.float32 and v.shape == (256,) and not v.any()
    sc = np.load(tmp_path / "a" / "mulvec_scalars.npy")
    pick = np.load(tmp_path / "a" / "mulvec_scalars_proofs.npy").astype(np.int64)
    assert sc.dtype == np.float64 and sc.shape[0] == pick.size == 256 and sc.shape[2] == 8 and sc.any()
    line2 = _plain_run(tmp_path / "b")
    assert line2["steps"] == 3
    assert np.array_equal(np.load(tmp_path / "b" / "verdicts.npy"), v)
    assert np.array_equal(np.load(tmp_path / "b" / "mulvec_scalars.npy"), sc)
    # the dumped scalars are the verifier's own: the same proofs (bench.py's seeded values, proved by the batched prover)
    # through the product API, MulVec scalars handed back by the pass
    sys.path.insert(0, ROOT)
    import bench
    import bulletproofsplus_amd as B
    from gpu_util import run_verifier_device
    a = B.Arith.init("bls12_381", 0)
    bv = B.BatchVerifier(B.PublicKey.new(a, 64), 64, 1, window_bits=10)
    vals, gams = zip(*(bench.synth_values(int(d) * 17, 1) for d in pick[:8]))
    pts, scs, V = bv.prove_batch(list(vals), list(gams))
    ok, os_, _ = run_verifier_device(torch, bv, np.concatenate([pts, V], axis=1), scs, want_result=False)
    assert not ok.any() and sc.shape[1] == bv.msm_len
    assert np.array_equal(os_.view(np.uint32).astype(np.float64), sc[:8])
