"""-m gpu: `bench.py --dump-outputs DIR` writes what the last timed step handed its caller -- per batch the verdict and status of the verify path, per
blob the commitment or proof and status of the commitment and proof paths -- as float32 .npy files, and the same arguments give the same files.  The
points are checked against the CPU oracle.  Every step of a run has the same inputs, so the verdicts of an honest verify step are all true whichever
step is dumped; the commitment and proof dumps are what ties the files to the step's own buffers.  Small launch sets and the 8-bit MSM table keep each
run to seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-host-leg", "--no-msm-legs", "--no-latency"]


def _bench(out_dir, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KZG355_BENCH_ECHO")}
    env["KZG355_MSM_BITS"] = "8"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(args) + ["--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2
    return line, {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_verify_dump_is_the_verdicts_of_the_last_step(tmp_path):
    _, got = _bench(tmp_path, "--batches-per-step", "5")
    assert sorted(got) == ["status", "verdicts"]
    assert all(a.dtype == np.float32 and a.shape == (5,) for a in got.values())
    assert np.all(got["verdicts"] == 1) and np.all(got["status"] == 0)


def test_commit_dump_is_the_commitments_and_the_same_from_run_to_run(tmp_path, oracle, oracle_settings):
    from synth import random_blob
    _, a = _bench(tmp_path / "a", "--op", "commit", "--batches-per-step", "2")
    _, b = _bench(tmp_path / "b", "--op", "commit", "--batches-per-step", "2")
    assert sorted(a) == ["commitments", "status"]
    assert a["commitments"].dtype == np.float32 and a["commitments"].shape == (128, 48) and a["status"].shape == (128,)
    assert np.all(a["status"] == 0)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # the first 64 blobs of the step are tests/synth.random_blob(0 .. 63)
    for i in (0, 63):
        assert bytes(a["commitments"][i].astype(np.uint8)) == oracle.blob_to_kzg_commitment(random_blob(i), oracle_settings), i


def test_proof_dump_is_the_proofs_of_the_step(tmp_path, oracle, oracle_settings):
    from synth import random_blob
    _, got = _bench(tmp_path, "--op", "proof", "--batches-per-step", "2")
    assert sorted(got) == ["proofs", "status"]
    assert got["proofs"].dtype == np.float32 and got["proofs"].shape == (128, 48) and np.all(got["status"] == 0)
    for i in (0, 1, 63):
        blob = random_blob(i)
        c = oracle.blob_to_kzg_commitment(blob, oracle_settings)
        assert bytes(got["proofs"][i].astype(np.uint8)) == oracle.compute_blob_kzg_proof(blob, c, oracle_settings), i
    assert len({bytes(r.astype(np.uint8)) for r in got["proofs"]}) == 128          # one proof per blob, not one row repeated


def test_every_exchange_form_is_timed_and_the_best_ones_step_is_dumped(tmp_path):
    """--sharded-path --exchange both on one GPU: the loop over the three exchange forms of a multi-GPU run (one timed region each, back to back) with
    --dump-outputs, without torch.distributed."""
    line, got = _bench(tmp_path, "--sharded-path", "--exchange", "both", "--batches-per-step", "3")
    cfg = dict(line["config"], **line["config"].get("detail", {}))
    assert cfg["skipped_for_time"] == "nothing"
    assert cfg["value_exchange"] in ("allgather", "allgather_split", "alltoall")
    for m in ("allgather", "allgather_split", "alltoall"):
        assert cfg[f"{m}_blobs_per_s"] > 0, m
    assert sorted(got) == ["status", "verdicts"] and got["verdicts"].shape == (3,)
    assert np.all(got["verdicts"] == 1) and np.all(got["status"] == 0)
