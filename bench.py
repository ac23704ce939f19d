#!/usr/bin/env python3
"""bench.py -- headline benchmark: blobs/sec on verify_blob_kzg_proof_batch (mainnet N=4096, batch = 64 per GPU).

Restates benches/kzg_benches.rs:93-126 (criterion group `verify_blob_kzg_proof_batch`, Throughput::Elements(n)):
  * inputs (benches/kzg_benches.rs:7-44): 64 random canonical blobs per batch, honest commitments and proofs made with
    the library itself (untimed setup), so every verification returns true -- asserted for every step;
  * the unit of work is one verify_blob_kzg_proof_batch call over a 64-blob batch (BASELINE.json configs[3]); at N GPUs
    the batch is 64*N blobs sharded 64 per rank with one all-to-all of the 160-byte records (configs[4]);
  * a STEP is one pass of the hot path (one set of kernel launches) over the step's synthetic input: G independent
    64-blob batches (`--batches-per-step G`), submitted together through kzg355_verify_blob_kzg_proof_batch_many_device
    (or the two stage functions around the exchange for N > 1).  One 64-blob batch is a chain of latency-bound integer
    kernels that occupies a handful of the chip's 1024 SIMDs, so whole-job throughput needs many batches in flight;
  * `value` is measured with the inputs resident in HBM when the timed region starts.

A plain run does only what `value` needs: the untimed setup, the warm-up, the timed steps, `--dump-outputs` and the line, with `roofline`
(HBM bound of the dominant kernel plus `roofline.alu`, the integer-issue bound that actually binds this path) from the HIP events of the
timed steps.  `--full` adds every leg that is measured or checked beside it: the single-batch latency, `config.host_inputs` (what the
reference's own bench shape gives: host slices through the drop-in C ABI, PCIe H2D inside the call), the mid-size and mixed legs, the
commitment / proof legs, the measured stream-copy rate, `cpu_baseline` and, for N > 1, the parity gate and the in-library leg -- never `value`.

Prints ONE JSON line on rank 0 (contract in the task statement).
`--sweep` restates the criterion sweep n in {1,2,4,8,16,32,64} and the five single-op benches (kzg_benches.rs:46-126).
"""
import argparse
import ctypes as C
import glob
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_PER_BATCH = 64
BLOB = 131072
HBM_PEAK_GBPS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
N_SIMD = 1024               # 256 CUs x 4 SIMD-32
NOMINAL_CLOCK_HZ = 2.4e9
# nominal VALU issue peak: one wave64 instruction per 2 cycles per SIMD-32 (MI355X_MICROARCH.md constants table, v_fma_f32)
NOMINAL_WAVE_INSTS_PER_S = N_SIMD * NOMINAL_CLOCK_HZ / 2
# Algorithmic bytes per blob, per kernel family (DESIGN.md "kernels" table); whole path per SURVEY.md 8(d): 262,240 B/blob.
PATH_BYTES_PER_BLOB = 131072 + 131072 + 48 + 48
KERNEL_BYTES_PER_BLOB = {
    "challenge": 16 + 16 + 131072 + 48 + 32,          # the 131,152-byte transcript in, z out
    "challenge_from_digest": 32 + 48 + 48 + 160,      # small host-buffer calls: the digest hashed on the host in, the record's C / z / proof fields out
    "decompress_points": 96,
    "eval": 131072 + 1364 * 36 + 32 + 32,             # blob + the 1364 inverse node roots of the radix-4 tree (eval_core.h) + z in, y out
    "validate_points": 96,
    "points_from_records": 96,
    "rpowers": 160 + 64,
    "lincomb": 2 * 112 + 64 + 2 * 112 / N_PER_BATCH,
    "lincomb_prep": 2 * 112 + 64, "lincomb_horner": 2 * 26 * 16 * 168 / N_PER_BATCH,
    "lincomb_shift": 2 * 112 + 2 * 26 * 168,          # few batches only: the 26 window shifts of every input point (side stream, under the hash)
    "pairing": (2 * 68 * 3 * 2 * 56 + 2 * 112) / N_PER_BATCH,   # two 68-line tables + two points per batch
}
# algorithmic bytes are independent of expanded precompute tables -- the wide-table MSM is priced at the B_commit
# figure (affine G1 sweep + scalars + output); the 11.7 MB of table rows it actually gathers per blob is `traffic`.
B_COMMIT = 4096 * (96 + 32) + 48
B_PROOF = 131072 + 131072 + 393216 + 48 + 48
KERNEL_BYTES_PER_BLOB.update({
    "msm_bucket": B_COMMIT,
    "msm_wide": B_COMMIT,
    "msm_finalize": 32 * 168 + 48,
    "digits": 131072 + 131072,
    "quotient": 131072 + 131072 + 131072,            # blob + roots sweep in, the quotient in the blob format out (rounds 1-4: 147,456 B of Montgomery limbs)
})
FAMILIES = list(KERNEL_BYTES_PER_BLOB)
PER_BATCH_FAMILIES = ("rpowers", "lincomb", "lincomb_prep", "lincomb_horner", "pairing", "points_from_records")
OP_BYTES_PER_BLOB = {"verify": PATH_BYTES_PER_BLOB, "commit": B_COMMIT, "proof": B_PROOF}
OP_METRIC = {"verify": "blobs/sec on verify_blob_kzg_proof_batch (mainnet 4096, batch=64)",
             "commit": "blobs/sec on blob_to_kzg_commitment (mainnet 4096-point G1 MSM)",
             "proof": "blobs/sec on compute_blob_kzg_proof (mainnet 4096)"}
KERNEL_NAMES = {"eval": ["k_eval"], "challenge": ["k_challenge_1w", "k_challenge"], "lincomb": ["k_lc_buckets", "k_lc_carry"], "lincomb_prep": ["k_lc_prep"],
                "lincomb_horner": ["k_lc_wsum", "k_lc_hchain_quad", "k_lc_horner"], "lincomb_shift": ["k_ps_shift"], "pairing": ["k_pairing_coop<3>", "k_pairing_hard12"], "validate_points": ["k_validate_points"], "rpowers": ["k_rhash_lanes", "k_rpowers"],
                "points_from_records": ["k_points_from_records"], "msm_bucket": ["k_msm_bucket<4>", "k_msm_bucket<1>"],
                "msm_wide": ["k_msm_wide_glv<false>", "k_msm_wide_glv<true>", "k_msm_wide<false>", "k_msm_wide<true>"], "quotient": ["k_quotient_tree<4>", "k_quotient_tree<2>", "k_quotient_tree<6>", "k_quotient_prep", "k_quotient_scan", "k_quotient"], "msm_finalize": ["k_msm_finalize"]}
ALTERNATIVE_FORMS = ("challenge", "msm_bucket", "msm_wide")     # lists of alternative forms of one kernel, not sequences


class PowerSampler:
    """Shader clock and socket power of this rank's GPU from its hwmon files (amdgpu: freq1_input = sclk in Hz, power1_input = PPT in
    microwatts, power1_cap), sampled every 10 ms by a thread while the timed steps run (the main thread sits in a ctypes call with the GIL
    released).  Best effort: any missing file turns it off.  On the MI355X boxes measured the verify path sits at the 1400 W cap with the
    shader clock around 2.28 of 2.4 GHz -- the card, not the kernel, picks the clock."""
    def __init__(self, dev_index):
        import threading
        self.ok, self.samples, self._stop, self._thread = False, [], threading.Event(), None
        try:
            import torch
            pr = torch.cuda.get_device_properties(dev_index)
            bdf = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
            hw = glob.glob(f"/sys/bus/pci/devices/{bdf}/hwmon/hwmon*")
            if not hw:
                return
            self.f_clk, self.f_pow, f_cap = hw[0] + "/freq1_input", hw[0] + "/power1_input", hw[0] + "/power1_cap"
            self.cap_w = int(open(f_cap).read()) / 1e6 if os.path.exists(f_cap) else None
            int(open(self.f_clk).read()); int(open(self.f_pow).read())
            self.ok = True
        except Exception:
            self.ok = False

    def _run(self):
        while not self._stop.is_set():
            try:
                self.samples.append((int(open(self.f_clk).read()) / 1e6, int(open(self.f_pow).read()) / 1e6))
            except Exception:
                pass
            self._stop.wait(0.01)

    def start(self):
        if self.ok:
            import threading
            self._thread = threading.Thread(target=self._run, daemon=True); self._thread.start()

    def stop(self):
        if not self._thread:
            return None
        self._stop.set(); self._thread.join(timeout=1.0)
        if len(self.samples) < 3:
            return None
        clk = sorted(c for c, _ in self.samples); pw = sorted(w for _, w in self.samples)
        q = lambda v, f: round(v[min(len(v) - 1, int(f * len(v)))], 1)
        return {"samples": len(self.samples), "interval_ms": 10, "sclk_mhz": {"median": q(clk, 0.5), "p10": q(clk, 0.1), "p90": q(clk, 0.9)},
                "socket_power_w": {"median": q(pw, 0.5), "p10": q(pw, 0.1), "p90": q(pw, 0.9)}, "power_cap_w": self.cap_w,
                "source": "amdgpu hwmon freq1_input / power1_input of this GPU, sampled over the timed steps",
                "note": "nominal-issue fractions in roofline.alu are priced at 2.4 GHz; at the clock the card actually sustains under its power cap they are 2400 / sclk higher"}


_REAL_STDOUT = None


def emit(line):
    """the run's ONE JSON line, to the process's real stdout (main() points file descriptor 1 at stderr for everything else)"""
    sys.stdout.flush()
    data = (json.dumps(line) + "\n").encode()
    fd = _REAL_STDOUT if _REAL_STDOUT is not None else 1
    while data:
        data = data[os.write(fd, data):]


DUMP_MAX_BYTES = 64 << 20
DUMP_SAMPLE_SEED = 0x4844


def dump_outputs(path, arrays):
    """--dump-outputs: every array as path/<name>.npy in float32 (bytes, verdicts and status codes are small integers, exact in float32).  The arrays
    share their first axis (one row per batch or per blob).  Past DUMP_MAX_BYTES in all, the same fixed, seeded sample of rows is kept of each, in row
    order, and sample_rows.npy (float64) names the rows; two runs with the same arguments sample the same rows."""
    import numpy as np
    arrays = {name: np.asarray(a).astype(np.float32) for name, a in arrays.items()}
    rows = len(next(iter(arrays.values())))
    assert all(len(a) == rows for a in arrays.values()), {name: a.shape for name, a in arrays.items()}
    row_bytes = sum(a.nbytes for a in arrays.values()) // max(rows, 1)
    keep = min(rows, DUMP_MAX_BYTES // (row_bytes + 8))
    os.makedirs(path, exist_ok=True)
    sample = os.path.join(path, "sample_rows.npy")
    if keep < rows:
        idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(rows, size=keep, replace=False))
        arrays = {name: a[idx] for name, a in arrays.items()}
        np.save(sample, idx.astype(np.float64))
    elif os.path.exists(sample):
        os.remove(sample)                                          # (left by an earlier, larger dump into the same directory)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    sys.stderr.write(f"bench.py: --dump-outputs: {', '.join(f'{n}{list(a.shape)}' for n, a in arrays.items())} -> {path}"
                     + (f" ({keep} of {rows} rows)\n" if keep < rows else "\n"))


def launcher_command(n, argv, port):
    """The command the driver itself uses for N > 1 (task statement): one rank per GPU under torch.distributed.run, rendezvous on 127.0.0.1."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(port),
            os.path.abspath(__file__)] + list(argv)


def launch_ranks(n, argv):
    """Start the N ranks of `bench.py --gpus N` as a child torch.distributed.run, relay rank 0's JSON line on stdout (everything else the
    ranks print goes to stderr) and return the child's exit code.  Called before this process has imported torch or touched the GPU."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")            # dmabuf IPC: RCCL across processes needs it on these hosts
    env.setdefault("OMP_NUM_THREADS", "8")
    import signal
    child = subprocess.Popen(launcher_command(n, argv, port), stdout=subprocess.PIPE, env=env, text=True, bufsize=1)

    # a launcher that is interrupted or terminated (a harness timeout sends SIGTERM) must not leave torchrun and its N GPU ranks behind
    # holding the cards: the signal is FORWARDED to the child (torchrun ends its ranks), the relay loop then sees EOF, and whatever ends the loop the
    # finally clause does not return while the child is alive.
    def forward(signum, frame):
        try:
            child.send_signal(signum)
        except Exception:
            pass
    old_handlers = {sg: signal.signal(sg, forward) for sg in (signal.SIGTERM, signal.SIGINT)}
    lines = 0
    try:
        for ln in child.stdout:
            is_line = False
            if ln.startswith("{"):
                try:
                    is_line = "metric" in json.loads(ln)
                except ValueError:
                    is_line = False
            if is_line:
                lines += 1
                sys.stdout.write(ln); sys.stdout.flush()
            else:
                sys.stderr.write(ln); sys.stderr.flush()
        rc = child.wait()
    finally:
        for sg, h in old_handlers.items():
            signal.signal(sg, h)
        if child.poll() is None:
            child.terminate()
            try:
                child.wait(timeout=20)
            except subprocess.TimeoutExpired:
                child.kill(); child.wait()
    if rc == 0 and lines != 1:
        sys.stderr.write(f"bench.py launcher: expected one JSON line from rank 0, saw {lines}\n")
        return 1
    return rc if rc >= 0 else 128 - rc                          # killed by a signal: shell convention


T_PROCESS_START = time.perf_counter()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batches-per-step", "--concurrent", dest="concurrent", type=int, default=None,
                    help="independent 64-blob batches verified by one step (one launch set)")
    ap.add_argument("--op", choices=["verify", "commit", "proof"], default="verify",
                    help="verify = the headline metric; commit / proof = secondary single-GPU metrics (BASELINE.json configs[1], [2])")
    ap.add_argument("--host-inputs", action="store_true",
                    help="time the host-buffer drop-in entry point (H2D over PCIe inside the timed region); never the headline value")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beside the headline figure: single-batch latency, host-input / mid-size / mixed legs, the commitment / proof legs, "
                         "the stream-copy rate, the CPU baseline and, N > 1, the parity gate and the in-library leg (a plain run: setup, warm-up, timed steps, line)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-host-leg", action="store_true", help="--full: skip the config.host_inputs measurements and the mid-size leg")
    ap.add_argument("--no-msm-legs", action="store_true", help="--full: skip the commitment / proof legs and the mixed leg (BASELINE configs[1], [2])")
    ap.add_argument("--no-latency", action="store_true", help="--full: skip the single-batch latency calls (profiling runs: every launch is then a full-size one)")
    ap.add_argument("--no-kernel-timing", action="store_true", help="no HIP events around the kernels of the timed region (A/B of their cost; no roofline)")
    ap.add_argument("--sharded-path", action="store_true",
                    help="run the multi-GPU code path (two-stage HipEngine driver of sharded.py) even at world size 1")
    ap.add_argument("--pipeline", type=int, default=1,
                    help="launch sets in flight (device-resident verify, 1 GPU): >1 submits every step with kzg355_verify_blob_kzg_proof_batch_many_device_submit and "
                         "collects the oldest once this many are queued -- mid-size sets (--batches-per-step 1024) kept in flight from one thread")
    ap.add_argument("--exchange", choices=["both", "alltoall", "allgather", "allgather_split"], default=os.environ.get("KZG355_BENCH_EXCHANGE", "both"),
                    help="N > 1: both (default) = K timed steps of EVERY form back to back, `value` = the best one (config.value_exchange names it); "
                         "alltoall = stage 2 split by batch; allgather = BASELINE north_star's single all-gather with stage 2 replicated; "
                         "allgather_split = the same all-gather with stage 2 split by batch")
    ap.add_argument("--no-parity-gate", action="store_true", help="N > 1, --full: skip the byte-exact check of the sharded path on the real ranks before the timed steps")
    ap.add_argument("--no-in-library-leg", action="store_true", help="N > 1, --full: skip the timing of the library's own multi-device handle (kzg355_load_trusted_setup_devices) on rank 0")
    ap.add_argument("--max-seconds", type=float, default=480.0,
                    help="wall-clock budget of the whole run from process start (the driver allows 600 s): optional legs are DROPPED, not cut short, once the time "
                         "left does not cover them -- N > 1: first the in-library leg, then the exchange forms beyond the first (north_star's all-gather always "
                         "runs); N = 1: the CPU all-threads trials, the mixed / mid-size legs.  config.skipped_for_time names what was dropped")
    ap.add_argument("--sweep", action="store_true",
                    help="criterion sweep: verify_blob_kzg_proof_batch for n in {1,..,64} and the five single-op benches, single calls on host inputs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step handed its caller as DIR/<name>.npy (float32; verify: verdicts and status per "
                         "batch, commit / proof: the 48-byte points and status per blob; past 64 MB a fixed, seeded sample of rows, see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and args.sweep:
        ap.error("--dump-outputs dumps the timed steps of the headline path; --sweep has none")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` the way the N = 1 run is started: this process becomes the launcher.  It has made no GPU call and
        # imported neither torch nor libkzg355.so; the N ranks are CHILD processes (no exec of a process that has touched the GPU).
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))
    # ONE JSON line on stdout, whatever the libraries under this process print: RCCL announces its version on STDOUT when a communicator is created, gloo
    # reports its connections there -- so file descriptor 1 is pointed at stderr for the life of the run and the line goes to the real stdout at the end.
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)
    if os.environ.get("KZG355_BENCH_ECHO"):
        # test hook (tests/test_bench_launcher.py, no GPU): every rank reports how it was started; rank 0 prints the line
        if rank == 0:
            emit({"metric": "echo", "argv": sys.argv[1:], "world": world, "gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
                  "exchange": args.exchange, "master_addr": os.environ.get("MASTER_ADDR"), "dump_outputs": args.dump_outputs,
                  "full": args.full})
        time.sleep(float(os.environ.get("KZG355_BENCH_ECHO_SLEEP", "0")))      # (test hook: ranks that stay up long enough to be interrupted)
        raise SystemExit(int(os.environ.get("KZG355_BENCH_ECHO_RC", "0")) if rank == world - 1 else 0)
    # Rehearsal hook (never set by the driver): KZG355_BENCH_FORCE_DIST=1 with one rank under torch.distributed.run makes the N = 1 run take the N > 1 code path --
    # process group on the real backend (nccl = RCCL), parity gate, both exchange forms through their collectives, the in-library leg -- on the one-GPU box:
    # RCCL refuses two ranks on one card, so a one-rank group is as much of the nccl path as that box can exercise.
    multi = world > 1 or (bool(os.environ.get("KZG355_BENCH_FORCE_DIST")) and "WORLD_SIZE" in os.environ)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: start N ranks with `python bench.py --gpus N` or torch.distributed.run --nproc-per-node N")
    import torch
    import torch.distributed as dist
    if world > 1 and not os.environ.get("KZG355_BENCH_ONE_GPU") and torch.cuda.device_count() < world:
        # fail fast, with one clear line, before any rank enters a rendezvous it cannot finish (device_count does not initialise the GPU)
        sys.stderr.write(f"bench.py: --gpus {world} but only {torch.cuda.device_count()} GPU(s) are visible to rank {rank}\n")
        raise SystemExit(3)
    # Rehearsal hooks for a one-GPU box (never set by the driver): KZG355_BENCH_BACKEND=gloo and KZG355_BENCH_ONE_GPU=1 run the N-rank
    # code path (sharding, the all-to-all, the status merge, max-over-ranks timing) with every rank on device 0; the line says so.
    backend = os.environ.get("KZG355_BENCH_BACKEND", "nccl")
    rehearsal = backend != "nccl" or bool(os.environ.get("KZG355_BENCH_ONE_GPU")) or (multi and world == 1)
    if os.environ.get("KZG355_BENCH_ONE_GPU"):
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    os.environ.setdefault("KZG355_DEVICE", str(local_rank))
    if multi:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import datetime
        try:
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=dev, timeout=datetime.timedelta(seconds=180))
                probe = torch.ones(1, device=dev)
                dist.all_reduce(probe)                              # the communicator is created here: an RCCL that cannot initialise fails NOW, not in the timed steps
                torch.cuda.synchronize()
                assert int(probe.item()) == world
            else:
                dist.init_process_group(backend, timeout=datetime.timedelta(seconds=180))
        except Exception as e:  # noqa: BLE001
            sys.stderr.write(f"bench.py: rank {rank}: torch.distributed / RCCL initialisation failed over {world} ranks: {e!r}\n")
            raise SystemExit(4)
        parking = dist.new_group(backend="gloo") if backend == "nccl" else None      # host-side barriers (the in-library leg parks the other ranks off their GPUs)
    if args.op != "verify":
        # commit / proof are bound by the fixed-base MSM: 16-bit windows over the GLV halves of the scalars (8 windows per half = 16 table rows per
        # scalar, 143.5 GB table) -- a handle left to itself sizes the table from half of the free HBM (15-bit: 18 rows, 68.9 GB, on an empty
        # card); a deployment that serves commitments sets the same knob (kzg355_options.msm_bits).  The verify path never reads the table.
        os.environ.setdefault("KZG355_MSM_BITS", "16")
    import kzg_rust_amd as kz
    from synth import random_blob
    L = kz.kzg.lib()

    golden = os.path.join(ROOT, "tests", "golden")
    g1 = open(os.path.join(golden, "trusted_setup_g1.bin"), "rb").read()
    g2 = open(os.path.join(golden, "trusted_setup_g2.bin"), "rb").read()
    s = kz.Kzg.load_trusted_setup([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)])
    assert s.device == local_rank

    if args.sweep:
        line = run_sweep(args, kz, L, s, dev, random_blob)
        if rank == 0:
            emit(line)
        s.free()
        return

    K, W = args.steps, args.warmup
    skipped = []                                   # legs dropped for --max-seconds (config.skipped_for_time)

    def time_left():
        return args.max_seconds - (time.perf_counter() - T_PROCESS_START)
    if args.concurrent is None:
        # verify: 8192 batches = 524,288 blobs = 69 GB of the card's 288 GB per step, one launch set (the larger the set the better the
        # kernels run: 2048 batches 3.13 M blobs/s, 4096 3.44 M, 8192 3.63 M); MSM-bound ops and the PCIe-inclusive variant: 256 batches
        args.concurrent = 8192 if (args.op == "verify" and not args.host_inputs) else 256
    Cc = max(1, args.concurrent)
    n_local = N_PER_BATCH
    # ---- untimed setup: Cc distinct batches per step; this rank owns blobs [rank*64, rank*64+64) of each batch.
    # Bench recipe (benches/kzg_benches.rs:14-23): random bytes, byte 0 of every 32-byte element forced to 0.  The first
    # batch comes from the seeded splitmix64 stream of tests/synth.py (it is also the CPU baseline's input); the rest is
    # drawn on the device from a fixed-seed torch generator.
    n_blobs = Cc * n_local
    gen = torch.Generator(device=dev); gen.manual_seed(0x4844 + rank)
    t_blobs = torch.randint(0, 256, (n_blobs, BLOB // 32, 32), dtype=torch.uint8, device=dev, generator=gen)
    t_blobs[:, :, 0] = 0
    host = bytearray(n_local * BLOB)
    for i in range(n_local):
        host[i * BLOB:(i + 1) * BLOB] = random_blob(rank * n_local + i)
    t_blobs = t_blobs.reshape(-1).contiguous()
    t_blobs[:n_local * BLOB] = torch.frombuffer(host, dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    SL = 65536                                     # untimed setup in slices: the proof path keeps a 147 KB quotient per blob in flight
    out = C.create_string_buffer(48 * min(n_blobs, SL))
    st = (C.c_int * max(n_blobs, 1))()
    commitments = bytearray()
    for lo in range(0, n_blobs, SL):
        cnt = min(SL, n_blobs - lo)
        rc = L.kzg355_blob_to_kzg_commitment_many_device(out, st, t_blobs.data_ptr() + lo * BLOB, cnt, s.handle)
        assert rc == 0, rc
        commitments += out.raw[:48 * cnt]
    commitments = bytes(commitments)
    t_c = torch.frombuffer(bytearray(commitments), dtype=torch.uint8).to(dev)
    proofs = bytearray()
    for lo in range(0, n_blobs, SL):
        cnt = min(SL, n_blobs - lo)
        rc = L.kzg355_compute_blob_kzg_proof_many_device(out, st, t_blobs.data_ptr() + lo * BLOB, t_c.data_ptr() + lo * 48, cnt, s.handle)
        assert rc == 0, rc
        proofs += out.raw[:48 * cnt]
    proofs = bytes(proofs)
    t_p = torch.frombuffer(bytearray(proofs), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()

    ok = (C.c_bool * Cc)()
    stg = (C.c_int * Cc)()

    h_blobs = t_blobs.cpu().numpy() if args.host_inputs else None      # pageable host copy, as a caller of the drop-in API would hold
    from kzg_rust_amd.sharded import HipEngine, verify_blob_kzg_proof_batch_sharded
    engine = HipEngine(s)
    out48 = C.create_string_buffer(48 * n_blobs)

    exchange_acc = {}                              # stage / exchange wall times of the sharded path, accumulated over the timed steps (this rank)
    mode_now = ["alltoall" if args.exchange == "both" else args.exchange]      # the exchange the sharded steps take right now
    last_step = {}                                 # the buffers the latest step handed back, by reference (--dump-outputs copies them after the timed steps)

    def run_steps(g):
        """one launch set over g independent 64-blob batches; returns when the results are on the host."""
        nb = g * n_local
        if args.op == "commit":
            rc = L.kzg355_blob_to_kzg_commitment_many_device(out48, st, t_blobs.data_ptr(), nb, s.handle)
            assert rc == 0 and out48.raw[:48 * nb] == commitments[:48 * nb]
            last_step.update(rows=nb, points=out48, status=st)
        elif args.op == "proof":
            rc = L.kzg355_compute_blob_kzg_proof_many_device(out48, st, t_blobs.data_ptr(), t_c.data_ptr(), nb, s.handle)
            assert rc == 0 and out48.raw[:48 * nb] == proofs[:48 * nb]
            last_step.update(rows=nb, points=out48, status=st)
        elif not multi and args.host_inputs:
            rc = L.kzg355_verify_blob_kzg_proof_batch_many(ok, stg, h_blobs.ctypes.data_as(C.c_char_p), commitments, proofs, n_local, g, s.handle)
            assert rc == 0, rc
            assert bytes(ok)[:g] == b"\x01" * g, "a verification returned false on honest inputs"     # (one memcmp: a Python loop over 8192 verdicts costs ~1 ms per step)
            last_step.update(rows=g, verdicts=ok, status=stg)
        elif not multi and not args.sharded_path:
            rc = L.kzg355_verify_blob_kzg_proof_batch_many_device(ok, stg, t_blobs.data_ptr(), t_c.data_ptr(), t_p.data_ptr(), n_local, g, s.handle)
            assert rc == 0, rc
            assert bytes(ok)[:g] == b"\x01" * g, "a verification returned false on honest inputs"     # (one memcmp: a Python loop over 8192 verdicts costs ~1 ms per step)
            last_step.update(rows=g, verdicts=ok, status=stg)
        else:
            # stage 1 on the local shard -> ONE all-to-all of the 160-byte records + decoded points (RCCL over xGMI) -> stage 2 on this rank's share of the batches
            oks, sts = verify_blob_kzg_proof_batch_sharded(t_blobs[:nb * BLOB], t_c[:nb * 48], t_p[:nb * 48], n_local, g, engine, exchange=mode_now[0], timings=exchange_acc, force_exchange=multi and world == 1)
            assert all(oks) and not any(sts), "a verification returned false on honest inputs"
            last_step.update(rows=g, verdicts=oks, status=sts)

    def step_outputs():
        """what the latest step handed its caller, copied out of the reused buffers (--dump-outputs)"""
        import numpy as np
        n = last_step["rows"]
        if "points" in last_step:
            out = {"commitments" if args.op == "commit" else "proofs": np.frombuffer(last_step["points"].raw[:48 * n], dtype=np.uint8).reshape(n, 48)}
        else:
            out = {"verdicts": np.array(last_step["verdicts"][:n], dtype=np.uint8)}
        out["status"] = np.array(last_step["status"][:n], dtype=np.int64)
        return out

    def barrier():
        torch.cuda.synchronize()
        if multi:
            dist.barrier()
        torch.cuda.synchronize()

    # single-batch latency (--full: reported, not the metric)
    measure_latency = args.full and not args.no_latency
    lat = [float("nan")]
    if measure_latency:
        run_steps(1)
        lat = []
        for _ in range(5):
            barrier(); t0 = time.perf_counter(); run_steps(1); barrier(); lat.append((time.perf_counter() - t0) * 1e3)
    latency_ms = statistics.median(lat)

    # --pipeline D: one host thread keeps D launch sets in flight (submit / collect halves of the same entry point; every set on its own
    # stream of the handle, so the narrow tail of one set runs under the wide kernels of the next)
    pipeline = args.pipeline if (args.pipeline > 1 and args.op == "verify" and not multi and not args.host_inputs and not args.sharded_path) else 1
    pending, free_slots = [], [((C.c_bool * Cc)(), (C.c_int * Cc)()) for _ in range(pipeline)]

    def collect_oldest():
        tk, slot = pending.pop(0)
        rc = L.kzg355_verify_collect(tk, slot[0], slot[1])
        assert rc == 0, rc
        assert bytes(slot[0])[:Cc] == b"\x01" * Cc, "a verification returned false on honest inputs"
        last_step.update(rows=Cc, verdicts=slot[0], status=slot[1])
        free_slots.append(slot)

    def step_pipelined():
        tk = C.c_void_p()
        rc = L.kzg355_verify_blob_kzg_proof_batch_many_device_submit(C.byref(tk), t_blobs.data_ptr(), t_c.data_ptr(), t_p.data_ptr(), n_local, Cc, s.handle)
        assert rc == 0, rc
        pending.append((tk, free_slots.pop()))
        if len(pending) >= pipeline:
            collect_oldest()

    def one_step():
        if pipeline > 1:
            step_pipelined()
        else:
            run_steps(Cc)                              # synchronous: returns when this step's verdicts are on the host

    parity = None
    if multi and args.op == "verify" and args.full and not args.no_parity_gate:
        # the only place real-xGMI parity can ever be checked: the sharded path on the real ranks against the committed fixture / the single-device run
        parity = parity_gate(kz, L, s, engine, dev, torch, dist, random_blob, rank, world, backend)

    def timed_region(mode):
        """W untimed + exactly K timed steps of one exchange form between barriers; max over ranks.  Returns everything the line needs of it."""
        mode_now[0] = mode
        for _ in range(W):
            one_step()
        while pending:
            collect_oldest()
        L.kzg355_reset_kernel_stats(s.handle)
        exchange_acc.clear()
        s.set_kernel_timing(not args.no_kernel_timing)     # HIP events around every kernel, on its launch stream; the schedule is unchanged
        step_ms = []
        sampler = PowerSampler(dev.index if dev.index is not None else 0) if rank == 0 else None
        barrier()
        if sampler: sampler.start()
        t0 = time.perf_counter()
        tp = t0
        for _ in range(K):
            one_step()
            tn = time.perf_counter(); step_ms.append((tn - tp) * 1e3); tp = tn
        while pending:                                     # (pipelined: the sets still in flight belong to the K timed steps)
            collect_oldest()
        barrier()
        dt = time.perf_counter() - t0
        power = sampler.stop() if sampler else None
        s.set_kernel_timing(False)
        if multi:
            tt = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        # N > 1 (or --sharded-path): where a step's time goes on every rank -- stage 1, the exchange (collective + permute), stage 2, the
        # verdict merge -- so that a sub-linear scaling curve can be attributed
        exchange_stats = None
        if exchange_acc:
            mine = {k: round(v / K, 3) for k, v in exchange_acc.items()}
            per_rank = [mine]
            if multi:
                per_rank = [None] * world
                dist.all_gather_object(per_rank, mine)
            exchange_stats = {"mode": mode, "per_rank_ms_per_step": per_rank,
                              "exchange_ms": max(r.get("exchange_ms", 0.0) for r in per_rank), "stage1_ms": max(r.get("stage1_ms", 0.0) for r in per_rank),
                              "stage2_ms": max(r.get("stage2_ms", 0.0) for r in per_rank), "merge_ms": max(r.get("merge_ms", 0.0) for r in per_rank),
                              "note": "wall ms per step, max over ranks; alltoall: records + decoded points of each rank's share of the batches, then an all-reduce of "
                                      "the verdict words (merge_ms); allgather (BASELINE north_star): one all-gather, stage 2 replicated on every rank"}
        stats = {}
        for fam in FAMILIES:
            tot, cnt = C.c_double(), C.c_long()
            L.kzg355_kernel_ms_stats(s.handle, fam.encode(), C.byref(tot), C.byref(cnt))
            if cnt.value:
                stats[fam] = (tot.value, cnt.value)
        return {"mode": mode, "dt": dt, "step_ms": step_ms, "power": power, "exchange_stats": exchange_stats, "stats": stats,
                "blobs_per_s": K * Cc * n_local * world / dt, "outputs": step_outputs() if args.dump_outputs else None}

    sharded = multi or args.sharded_path
    modes = ["allgather", "allgather_split", "alltoall"] if (sharded and args.exchange == "both" and args.op == "verify") else [mode_now[0]]
    # (the same K and W for each form, back to back.  --max-seconds: a further form needs what the last one took, and the line, the parity of the exit and --
    # N > 1 -- the in-library leg's 20 s minimum still have to fit behind it; all ranks take the same decision from rank 0's clock)
    setup_s = time.perf_counter() - T_PROCESS_START                 # start to the first warm-up step (config.setup_s)
    runs = {}
    for m in modes:
        if runs:
            last = list(runs.values())[-1]["wall_s"]
            go = time_left() > 1.3 * last + 45.0
            if multi:
                flag = torch.tensor([1 if go else 0], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
                dist.broadcast(flag, src=0)
                go = bool(int(flag.item()))
            if not go:
                skipped.append(f"exchange form {m}")
                continue
        t_form = time.perf_counter()
        runs[m] = timed_region(m)
        runs[m]["wall_s"] = time.perf_counter() - t_form
    best = max(runs.values(), key=lambda r: r["blobs_per_s"])
    dt, step_ms, power, exchange_stats, stats = best["dt"], best["step_ms"], best["power"], best["exchange_stats"], best["stats"]
    value_exchange = best["mode"] if sharded else None
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, best["outputs"])

    blobs_total = K * Cc * n_local * world
    value = blobs_total / dt
    blobs_events = blobs_total

    # ---- roofline of the dominant kernel (HIP events recorded on the launch stream during the timed region)
    roofline = None
    if stats:
        dom = max(stats, key=lambda f: stats[f][0])
        tot_ms, cnt = stats[dom]
        avg_s = tot_ms / cnt / 1e3

        def blobs_per_launch_of(fam):
            if args.op != "verify":
                return Cc * n_local
            # stage 2 covers every rank's records only in the replicated form; in the split forms (all-to-all, split all-gather) a rank takes 1 / world of the batches
            replicated = fam in PER_BATCH_FAMILIES and (not sharded or value_exchange == "allgather")
            return blobs_events / stats[fam][1] if replicated else blobs_events / world / stats[fam][1]

        def insts_scale_of(fam):
            # the committed SQ pass is over 64-blob batches; a sharded batch has 64 x world records, so the kernels whose work is per BATCH (the pairing, the
            # window sums and chains of the linear combination) do 1 / world of that per record
            return 1.0 / world if sharded and fam in ("pairing", "lincomb_horner") else 1.0
        blobs_per_launch = blobs_per_launch_of(dom)
        achieved = KERNEL_BYTES_PER_BLOB[dom] * blobs_per_launch / avg_s / 1e9
        traffic, traffic_src = pmc_traffic(dom, blobs_per_launch, None if args.op == "verify" else args.op)
        roofline = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 3), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic, "traffic_unit": "bytes per launch (PMC FETCH_SIZE x2 + WRITE_SIZE)",
                    "traffic_source": traffic_src, "algorithmic_bytes_per_launch": KERNEL_BYTES_PER_BLOB[dom] * blobs_per_launch,
                    "avg_launch_ms": round(tot_ms / cnt, 4), "launches": cnt,
                    "kernel_timing": "HIP events on the launch stream around every kernel, recorded during the timed region",
                    "kernel_ms_share": {f: round(v[0], 3) for f, v in sorted(stats.items(), key=lambda kv: -kv[1][0])},
                    # every kernel family against the same HBM peak (algorithmic bytes per launch / its average launch duration): the dominant kernel above is
                    # the one with the most TIME, which need not be the one closest to the memory roofline
                    "per_kernel": {f: {"avg_launch_ms": round(v[0] / v[1], 4), "achieved_gbps": round(KERNEL_BYTES_PER_BLOB[f] * blobs_per_launch_of(f) / (v[0] / v[1] / 1e3) / 1e9, 1),
                                       "frac": round(KERNEL_BYTES_PER_BLOB[f] * blobs_per_launch_of(f) / (v[0] / v[1] / 1e3) / 1e9 / HBM_PEAK_GBPS, 4)}
                                   for f, v in sorted(stats.items(), key=lambda kv: -kv[1][0]) if f in KERNEL_BYTES_PER_BLOB},
                    "path_bytes_per_blob": OP_BYTES_PER_BLOB[args.op],
                    "path_frac_of_hbm_peak": value * OP_BYTES_PER_BLOB[args.op] / (world * HBM_PEAK_GBPS * 1e9),
                    "measured_stream_copy_gbps": stream_copy_peak(torch, dev) if rank == 0 and args.full else None,
                    "alu": alu_roofline(stats, blobs_per_launch_of, value / world, insts_scale_of) if args.op == "verify" else None,      # (the committed SQ pass is over the verify bench)
                    "note": "integer-issue-bound path (~1e3 integer ops per byte): the HBM fraction is small by construction; roofline.alu is the bound that binds"}
        if args.op != "verify" and s.msm_form >= 10:
            # the memory-side bound of the fixed-base MSM is not streaming bandwidth but RANDOM 128-byte row gathers: one table row per (window, scalar).
            # Measured ceiling of that access pattern on MI355X: tools/ubench/gather_rate.hip, profiles/r03/gather_rate_random_128B.txt
            bits, wins, glv, table_bytes = s.msm_shape()
            rows_per_blob = 4096 * ((2 * wins) if glv else (wins if bits != 15 else 17.45))      # GLV: two halves per scalar; 256-bit 15-bit form: 17 full windows and a carry window hit by 45 % of the scalars
            rows_per_s = rows_per_blob * value / world
            roofline["gather"] = {"rows_per_blob": round(rows_per_blob), "achieved_rows_per_s": rows_per_s, "achieved_gbps": round(rows_per_s * 128 / 1e9, 1),
                                  "measured_random_128B_gather_peak_gbps": 1427.0, "frac_of_gather_peak": round(rows_per_s * 128 / 1427.0e9, 4),
                                  "table": {"bits": bits, "windows_per_half_scalar" if glv else "windows": wins, "glv": bool(glv), "bytes": table_bytes},
                                  "source": "profiles/r03/gather_rate_random_128B.txt (11.1 G rows/s; streaming read of the same buffer: 5678 GB/s)"}

    host_inputs = None
    mid_size = None
    if rank == 0 and not multi and args.op == "verify" and not args.host_inputs and args.full and not args.no_host_leg:
        host_inputs = host_leg(L, s, t_blobs, commitments, proofs, n_local, min(Cc, 1024))
        if pipeline == 1 and Cc >= 1024 and not args.sharded_path:
            mid_size = mid_size_leg(L, s, t_blobs, t_c, t_p, n_local)
    cpu_baseline = None
    if rank == 0 and not multi and args.full and not args.no_cpu_baseline:
        cpu_baseline = time_cpu_baseline(args.op, commitments[:48 * n_local], proofs[:48 * n_local], host, n_local,
                                         match_threads=host_inputs.get("single_call_host_threads") if host_inputs else None,
                                         all_threads=time_left() > 200.0)
        if not cpu_baseline.get("all_cores"):
            skipped.append("CPU all-threads trials")

    coexist = None
    if rank == 0 and not multi and args.op == "verify" and not args.host_inputs and args.full and not args.no_msm_legs and not args.sharded_path and pipeline == 1 and Cc >= 1024:
        # what a drop-in KzgSettings serves -- verification AND commitments from ONE handle, nothing freed in between.  `s` is a default
        # handle: the untimed setup's commitments made it size its own table (from half of the HBM free at that moment), and the step's 69 GB of blobs are
        # still resident beside it.
        if time_left() > 150.0:
            coexist = coexist_leg(L, s, t_blobs, t_c, t_p, commitments, n_local, min(n_blobs, 16384))
        else:
            skipped.append("default-table / mixed leg")

    msm_form_at_end = s.msm_form
    msm_legs = None
    if rank == 0 and not multi and args.op == "verify" and not args.host_inputs and args.full and not args.no_msm_legs and not args.sharded_path:
        # BASELINE configs[1] and [2] in the same driver-timed run: the verify handle and its launch sets are released first (69 GB of blobs,
        # the table the untimed setup built), then a handle with the widest MSM table that fits serves both legs
        msm_form_verify_setup = s.msm_form
        n_leg = min(n_blobs, 16384)
        keep_b = t_blobs[:n_leg * BLOB].clone(); keep_c = t_c[:n_leg * 48].clone()
        s.free(); engine = None
        t_blobs = t_c = t_p = None
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        msm_legs = run_msm_legs(kz, L, torch, dev, g1, g2, keep_b, keep_c, commitments[:48 * n_leg], proofs[:48 * n_leg], n_leg)
        msm_legs["verify_setup_msm_form"] = msm_form_verify_setup
        s = None

    in_library = None
    run_in_library = multi and args.op == "verify" and args.full and not args.no_in_library_leg
    if run_in_library:
        # the first leg to go when time is short (it loads N handles and makes 256 commitments and proofs before it times anything: ~60-100 s on 8 devices)
        go = time_left() > float(os.environ.get("KZG355_BENCH_IN_LIBRARY_NEEDS", "150"))
        flag = torch.tensor([1 if go else 0], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
        dist.broadcast(flag, src=0)
        if not int(flag.item()):
            run_in_library = False
            skipped.append("in-library leg")
    if run_in_library:
        # The multi-GPU path a Rust / C caller actually gets: ONE handle over all N devices inside rank 0's process.  The other ranks
        # give their GPUs back first and wait on a HOST-side barrier (gloo) -- an RCCL barrier would keep a kernel spinning on every card.
        t_blobs = t_c = t_p = None
        engine = None
        s.free(); s = None
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        park = (lambda: dist.barrier(group=parking)) if parking is not None else dist.barrier
        park()
        hung = False
        if rank == 0:
            # The leg must never cost the run its line: an exception is reported in the line, and so is a HANG (an RCCL that deadlocks inside the library
            # cannot be cancelled) -- the leg runs on a daemon thread under a watchdog, and a run whose leg did not come back prints its line, lets the
            # other ranks go and leaves through os._exit.
            import threading
            box = {}

            def leg():
                try:
                    box["out"] = in_library_leg(kz, L, g1, g2, world, random_blob, one_gpu=bool(os.environ.get("KZG355_BENCH_ONE_GPU")))
                except Exception as e:  # noqa: BLE001
                    box["out"] = {"in_library_error": repr(e)[:300]}
            th = threading.Thread(target=leg, daemon=True)
            th.start()
            th.join(timeout=min(float(os.environ.get("KZG355_BENCH_IN_LIBRARY_TIMEOUT", "240")), max(20.0, time_left() - 15.0)))
            hung = th.is_alive()
            in_library = {"in_library_error": "timed out (the leg is still running; its thread was abandoned)"} if hung else box.get("out")
        park()

    if rank == 0:
        line = {
            "metric": OP_METRIC[args.op],
            "value": value, "unit": "blobs/s", "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": dt * 1e3 / K, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u32 limbs (29-bit) / 64-bit accumulate, u8 bytes", "data": "synthetic",
            "config": {"workload": ("kzg_mainnet verify_blob_kzg_proof_batch, 64 random blobs per GPU per batch, "
                                    + ("host buffers (PCIe H2D inside the timed region)" if args.host_inputs else "device-resident inputs (blobs in HBM when the timed region starts)")
                                    if args.op == "verify" else
                                    f"kzg_mainnet {'blob_to_kzg_commitment' if args.op == 'commit' else 'compute_blob_kzg_proof'}, independent blobs")
                                   + ("" if not multi else f", one batch of {64 * world} blobs sharded over {world} GPUs, "
                                      + {"alltoall": "all-to-all of the 160-B records + decoded points (stage 2 split by batch)",
                                         "allgather": "one all-gather of the 160-B records + decoded points (stage 2 replicated: BASELINE north_star's form)",
                                         "allgather_split": "one all-gather of the 160-B records + decoded points (BASELINE north_star's collective), stage 2 split by batch"}[value_exchange]),
                       "batch_size": n_local * world, "batches_per_step": Cc, "blobs_per_step": Cc * n_local * world,
                       "field_elements_per_blob": 4096, "sets_in_flight": pipeline, "inputs": "host buffers (PCIe H2D inside the timed region)" if args.host_inputs else "resident in HBM",
                       "msm_form": msm_legs["verify_setup_msm_form"] if msm_legs else msm_form_at_end, **({"rehearsal": f"{world} rank(s) on ONE GPU, backend {backend}: code-path check, not a measurement"} if rehearsal and multi else {}),
                       "step_ms": {"median": round(statistics.median(step_ms), 4), "min": round(min(step_ms), 4), "mean": round(dt * 1e3 / K, 4)},
                       "latency_ms_single_batch": round(latency_ms, 3) if measure_latency else None, "latency_ms_single_batch_min": round(min(lat), 3) if measure_latency else None,
                       "host_inputs": host_inputs, "mid_size_sets": mid_size, "power": power, "full": args.full},
            "roofline": roofline, "cpu_baseline": cpu_baseline,
        }
        if host_inputs:
            # the call at the drop-in boundary includes the H2D of the blobs.  `value` is the device-resident rate the task
            # statement asks for; these two are the H2D-inclusive rates of the same build, same run (details in config.host_inputs)
            line["value_host_single_call"] = host_inputs["single_call_blobs_per_s"]      # one verify_blob_kzg_proof_batch(n = 64) on host slices (benches/kzg_benches.rs:113-120)
            line["single_call_ms"] = host_inputs["single_call_ms"]
            line["value_host_stream"] = host_inputs["stream_blobs_per_s"]               # many batches streamed from pageable host memory by one *_many call
        if mid_size:
            line["value_mid_size_sets_in_flight"] = mid_size["blobs_per_s"]              # 1024-batch sets, three in flight (config.mid_size_sets)
        if exchange_stats:
            line["config"]["exchange"] = exchange_stats
        if sharded:
            # both exchange forms of the same run as scalars; `value` is the better one and says which (BASELINE config 5 / north_star name the all-gather)
            cfg = line["config"]
            cfg["value_exchange"] = value_exchange
            for m, r in runs.items():
                cfg[f"{m}_blobs_per_s"] = round(r["blobs_per_s"], 1)
                cfg[f"{m}_ms_per_step"] = round(r["dt"] * 1e3 / K, 3)
                for k in ("stage1_ms", "exchange_ms", "stage2_ms", "merge_ms"):
                    if r["exchange_stats"]:
                        cfg[f"{k}_{m}"] = r["exchange_stats"][k]
            if len(runs) > 1:
                cfg["exchange_by_mode"] = {m: r["exchange_stats"] for m, r in runs.items()}
        if parity:
            line["config"].update(parity)
        if in_library:
            line["config"].update(in_library)
        line["config"]["skipped_for_time"] = "; ".join(skipped) if skipped else "nothing"
        line["config"]["wall_s"] = round(time.perf_counter() - T_PROCESS_START, 1)      # this process, start to line (the launcher of an N > 1 run adds its own start-up)
        line["config"]["setup_s"] = round(setup_s, 1)
        flatten_scalars(line, host_inputs, mid_size, power, msm_legs, coexist, multi=multi)
        emit(line)
    if s is not None:
        s.free()
    if multi:
        dist.destroy_process_group()
        if rank == 0 and in_library and "timed out" in str(in_library.get("in_library_error", "")):
            sys.stdout.flush(); sys.stderr.flush()
            # the abandoned in-library thread is stuck in a device call: no orderly interpreter shutdown.  NON-ZERO: a deadlock inside the library's
            # own RCCL / peer-copy path is a failure the launcher, CI and the driver must see -- the line above still carries every measurement that finished
            os._exit(6)


def parity_gate(kz, L, s, engine, dev, torch, dist, random_blob, rank, world, backend):
    """N > 1, before anything is timed: ONE batch of 64 x N blobs -- the first 64 N blobs of the committed 512-blob fixture (tests/golden/batch512.json:
    tests/synth.random_blob(512000 + i), commitments and proofs from the CPU oracle) -- through the sharded path on the REAL ranks, both exchange forms:
      * verdict true; with two proofs swapped on rank 0: false;
      * the gathered records (C | z | y | proof of every blob, the body of the r-transcript in the order of utils.rs:454-463) byte for byte equal
        to what rank 0 computes for all 64 N blobs on its own device, and r / proof_lincomb / rhs of the gathered batch (kzg.rs:601-622) equal to the
        single-device run's -- and, at N = 8, to the fixture's own values (oracle-derived, committed).
    Any mismatch raises on rank 0 after a verdict word has been shared, so that every rank leaves together."""
    from kzg_rust_amd.sharded import verify_blob_kzg_proof_batch_sharded
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "batch512.json")))
    n_local, n = N_PER_BATCH, N_PER_BATCH * world
    if n > fx["n"]:
        return {"parity_gate": f"skipped: {n} blobs exceed the committed {fx['n']}-blob fixture"}
    first = fx["first_index"]
    lo = rank * n_local
    to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    tb = to_dev(b"".join(random_blob(first + lo + i) for i in range(n_local)))
    cs = [bytes.fromhex(c) for c in fx["commitments"][:n]]
    ps = [bytes.fromhex(p) for p in fx["proofs"][:n]]
    tc, tp = to_dev(b"".join(cs[lo:lo + n_local])), to_dev(b"".join(ps[lo:lo + n_local]))
    sw = list(ps[lo:lo + n_local])
    if rank == 0:
        sw[1], sw[2] = sw[2], sw[1]
    tsw = to_dev(b"".join(sw))
    torch.cuda.synchronize()
    problems = []
    gathered = None
    for mode in ("allgather", "allgather_split", "alltoall"):
        cap = {}
        ok, st = verify_blob_kzg_proof_batch_sharded(tb, tc, tp, n_local, 1, engine, exchange=mode, capture=cap, force_exchange=world == 1)
        if ok != [True] or st != [0]:
            problems.append(f"{mode}: honest batch gave {ok} / {st}")
        if mode == "allgather":
            gathered = cap.get("records")
        ok, st = verify_blob_kzg_proof_batch_sharded(tb, tc, tsw, n_local, 1, engine, exchange=mode, force_exchange=world == 1)
        if ok != [False] or st != [0]:
            problems.append(f"{mode}: swapped twin gave {ok} / {st}")
    out = {}
    try:
      if rank == 0:
        if gathered is None or gathered.numel() != 160 * n:
            problems.append("no gathered records captured")
        else:
            r_sh, pl_sh, rhs_sh, ok_sh, st_sh = engine.batch_intermediates(gathered, n, 1)[0]
            # the same batch, whole, on this rank's device alone
            all_b = to_dev(b"".join(random_blob(first + i) for i in range(n)))
            all_c, all_p = to_dev(b"".join(cs)), to_dev(b"".join(ps))
            rec = torch.empty(160 * n, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            st1 = (C.c_int * 1)()
            rc = L.kzg355_verify_shard_records_device(rec.data_ptr(), st1, all_b.data_ptr(), all_c.data_ptr(), all_p.data_ptr(), n, 1, s.handle)
            if rc != 0 or st1[0] != 0:
                problems.append(f"single-device stage 1 failed: {rc} / {st1[0]}")
            if bytes(rec.cpu().numpy()) != bytes(gathered.cpu().numpy()):
                problems.append("gathered records differ from the single-device records (transcript order / exchange)")
            r_1, pl_1, rhs_1, ok_1, st_1 = engine.batch_intermediates(rec, n, 1)[0]
            if (r_sh, pl_sh, rhs_sh, ok_sh, st_sh) != (r_1, pl_1, rhs_1, True, 0):
                problems.append("r / proof_lincomb / rhs of the sharded batch differ from the single-device run")
            if n == fx["n"] and (r_sh.hex(), pl_sh.hex(), rhs_sh.hex()) != (fx["r"], fx["proof_lincomb"], fx["rhs"]):
                problems.append("r / proof_lincomb / rhs differ from tests/golden/batch512.json")
            out = {"parity_gate": "passed" if not problems else "FAILED: " + "; ".join(problems), "parity_gate_blobs": n,
                   "parity_gate_r": r_sh.hex(), "parity_gate_against": ("tests/golden/batch512.json (oracle-derived r, proof_lincomb, rhs) and " if n == fx["n"] else "")
                   + "the single-device run of the same batch on rank 0: records, r, proof_lincomb, rhs byte-exact; verdicts true / false in all three exchange forms"}
    except Exception as e:  # noqa: BLE001
        # whatever rank 0's own comparison raises (an unexpected status out of batch_intermediates, a device error) is a PROBLEM of the gate, not an
        # exception of one rank: the others are already waiting in the all-reduce below and every rank must leave together with the one-line report
        problems.append(f"rank-0 comparison raised {e!r}")
    flag = torch.tensor([1 if problems else 0], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
    dist.all_reduce(flag, op=dist.ReduceOp.MAX)
    if int(flag.item()):
        if problems:
            sys.stderr.write(f"bench.py: rank {rank}: parity gate FAILED: {'; '.join(problems)}\n")
        raise SystemExit(5)
    return out


def in_library_leg(kz, L, g1, g2, world, random_blob, one_gpu=False, many_batches_per_device=128):
    """kzg355_load_trusted_setup_devices over all N devices in ONE process (rank 0), timed through the drop-in C ABI on host slices:
      (a) ONE verify_blob_kzg_proof_batch of 64 N blobs (BASELINE config 5 literally: per-device blocks of 64 blobs, stage 1 per block, the library's own
          ncclAllGather of the 160-byte records over xGMI -- or its peer-copy fallback, the line says which -- stage 2 on one device);
      (b) a *_many call of 128 N independent 64-blob batches fanned out over the devices (contiguous ranges, no exchange).
    Inputs: the committed fixture's first 64 N blobs (a) and seeded blobs with commitments / proofs made by the same handle (b).  Host memory in, PCIe inside
    the calls: these are drop-in figures, never `value`."""
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "batch512.json")))
    devices = [0] * world if one_gpu else list(range(world))
    t0 = time.perf_counter()
    # (msm_bits = 12: the leg makes 256 commitments and proofs for its inputs once -- the 10.9 GB table builds in a fraction of a second per device, the
    # 68.9 GB one a default handle would size from the free HBM takes seconds on each of N devices and serves nothing that is timed here)
    s = kz.KzgSettings.load_trusted_setup_ex([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)], devices=devices, msm_bits=12)
    load_s = time.perf_counter() - t0
    out = {"in_library_devices": s.device_count, "in_library_load_s": round(load_s, 2)}
    try:
        n = N_PER_BATCH * world
        first = fx["first_index"]
        blobs = b"".join(random_blob(first + i) for i in range(n))
        cs = b"".join(bytes.fromhex(c) for c in fx["commitments"][:n]); ps = b"".join(bytes.fromhex(p) for p in fx["proofs"][:n])
        ok = C.c_bool()
        ts = []
        kind0, ag0, peer0 = s.exchange_stats()
        for i in range(12):
            t0 = time.perf_counter()
            rc = L.kzg355_verify_blob_kzg_proof_batch(C.byref(ok), blobs, n, cs, n, ps, n, s.handle)
            ts.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0 and ok.value, (rc, ok.value)
        kind, ag, peer = s.exchange_stats()
        ts = ts[2:]
        out.update({"in_library_single_call_ms": round(statistics.median(ts), 3), "in_library_single_call_ms_min": round(min(ts), 3),
                    "in_library_single_call_blobs": n, "in_library_single_call_blobs_per_s": round(n / (statistics.median(ts) / 1e3), 1),
                    "in_library_exchange": "ncclAllGather (RCCL)" if ag > ag0 else "peer copies" if peer > peer0 else "none (not sharded)"})
        # (b) fan-out: G batches of 64; commitments and proofs from the handle itself
        G = many_batches_per_device * world
        nb = G * N_PER_BATCH
        import numpy as np
        hb = np.empty(nb * BLOB, dtype=np.uint8)
        base = np.frombuffer(b"".join(random_blob(900000 + i) for i in range(256)), dtype=np.uint8).reshape(256, BLOB)
        for k in range(0, nb, 256):                               # 256 distinct blobs tiled (every batch is honest; the verdicts do not depend on distinctness)
            m = min(256, nb - k)
            hb[k * BLOB:(k + m) * BLOB] = base[:m].reshape(-1)
        out48 = C.create_string_buffer(48 * 256); st = (C.c_int * 256)()
        assert L.kzg355_blob_to_kzg_commitment_many(out48, st, base.ctypes.data_as(C.c_char_p), 256, s.handle) == 0
        c256 = out48.raw
        assert L.kzg355_compute_blob_kzg_proof_many(out48, st, base.ctypes.data_as(C.c_char_p), c256, 256, s.handle) == 0
        p256 = out48.raw
        reps = (nb + 255) // 256
        hc, hp = (c256 * reps)[:48 * nb], (p256 * reps)[:48 * nb]
        okg = (C.c_bool * G)(); stg = (C.c_int * G)()
        rates = []
        for i in range(4):
            t0 = time.perf_counter()
            rc = L.kzg355_verify_blob_kzg_proof_batch_many(okg, stg, hb.ctypes.data_as(C.c_char_p), hc, hp, N_PER_BATCH, G, s.handle)
            dtm = time.perf_counter() - t0
            assert rc == 0 and bytes(okg) == b"\x01" * G, rc
            if i:
                rates.append(nb / dtm)
        out.update({"in_library_blobs_per_s": round(statistics.median(rates), 1), "in_library_many_batches": G,
                    "in_library_note": "ONE handle over all N devices in one process, host buffers through the drop-in C ABI (PCIe inside the calls): single_call = one "
                                       "verify_blob_kzg_proof_batch of 64 N blobs (config 5's shape); blobs_per_s = one *_many call of 128 N batches of 64 fanned out over the devices"})
    finally:
        s.free()
    return out


def run_msm_legs(kz, L, torch, dev, g1, g2, t_blobs, t_c, commitments, proofs, n, steps=6, warmup=2):
    """BASELINE configs[1] / [2] inside the default run: blob_to_kzg_commitment and compute_blob_kzg_proof over n independent device-resident blobs
    per launch (benches/kzg_benches.rs:46-91 time one call each; here one launch set of n blobs is a step, as for `value`).  The handle is loaded
    for the widest fixed-base table that fits the card now that the verify launch sets are gone (16-bit GLV windows = 143.5 GB when >= 160 GB are free,
    else what the handle picks from half of the free HBM); every step's outputs are compared with the untimed setup's (made with ANOTHER table
    width: the two forms must agree byte for byte).  `north_star`'s "fraction of the HBM-read roofline for the G1 trusted-setup sweep" is
    g1_sweep_hbm_frac: SURVEY 8d's B_commit / B_proof bytes per blob x blobs/s over the 8 TB/s peak; traffic_over_algorithmic says what the wide table
    really moves (committed PMC passes of `bench.py --op commit|proof`), gather_frac prices it against the measured random-128-B-row gather ceiling."""
    free_b, total_b = torch.cuda.mem_get_info(dev)
    want16 = free_b >= 160 * (1 << 30)
    t0 = time.perf_counter()
    s = kz.KzgSettings.load_trusted_setup_ex([g1[48 * i:48 * i + 48] for i in range(4096)], [g2[96 * i:96 * i + 96] for i in range(65)],
                                             device=dev.index or 0, msm_bits=16 if want16 else 0)
    s.build_msm_table()
    build_s = time.perf_counter() - t0
    bits, wins, glv, table_bytes = s.msm_shape()
    out48 = C.create_string_buffer(48 * n)
    st = (C.c_int * n)()
    legs = {"blobs_per_launch": n, "steps": steps, "msm_bits": bits, "msm_glv": bool(glv), "table_gb": round(table_bytes / 1e9, 1), "table_build_s": round(build_s, 2),
            "free_hbm_gb_before_table": round(free_b / 1e9, 1)}
    rows_per_blob = 4096 * ((2 * wins) if glv else (wins if bits != 15 else 17.45)) if bits >= 10 else None
    for op in ("commit", "proof"):
        def step():
            if op == "commit":
                rc = L.kzg355_blob_to_kzg_commitment_many_device(out48, st, t_blobs.data_ptr(), n, s.handle)
                assert rc == 0 and out48.raw[:48 * n] == commitments, "commitments differ between the two table forms"
            else:
                rc = L.kzg355_compute_blob_kzg_proof_many_device(out48, st, t_blobs.data_ptr(), t_c.data_ptr(), n, s.handle)
                assert rc == 0 and out48.raw[:48 * n] == proofs, "proofs differ between the two table forms"
        for _ in range(warmup):
            step()
        L.kzg355_reset_kernel_stats(s.handle)
        s.set_kernel_timing(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        s.set_kernel_timing(False)
        rate = steps * n / dt
        kms = {}
        for fam in FAMILIES:
            tot, cnt = C.c_double(), C.c_long()
            L.kzg355_kernel_ms_stats(s.handle, fam.encode(), C.byref(tot), C.byref(cnt))
            if cnt.value:
                kms[fam] = round(tot.value / cnt.value, 4)
        b_alg = OP_BYTES_PER_BLOB[op]
        traffic = 0.0
        src = None
        for fam in kms:
            tr, f = pmc_traffic(fam, 1, op)
            if tr:
                traffic += tr; src = f
        d = {"blobs_per_s": round(rate, 1), "ms_per_launch": round(dt * 1e3 / steps, 3), "kernel_ms": kms,
             "algorithmic_bytes_per_blob": b_alg, "g1_sweep_hbm_frac": round(rate * b_alg / (HBM_PEAK_GBPS * 1e9), 5),
             "traffic_bytes_per_blob": round(traffic) if traffic else None, "traffic_over_algorithmic": round(traffic / b_alg, 2) if traffic else None, "traffic_source": src}
        # the MSM kernel (and the quotient kernel of the proof leg) against the floor of its own instruction mix, as roofline.alu does for the verify kernels
        mix_files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "inst_mix.json")))
        mix = json.load(open(mix_files[-1]))["per_kernel"] if mix_files else {}
        for fam, key in (("msm_wide", "msm"), ("quotient", "quotient")):
            if fam not in kms:
                continue
            f, per = newest_profile("sq", KERNEL_NAMES[fam], op)
            cands = [k for k in KERNEL_NAMES[fam] if per and k in per and k in mix]
            if op == "proof" and fam == "msm_wide":
                cands = [k for k in cands if "true" in k] or cands     # the quotient arrives as scalars in the blob format since round 5: <false> either way; keep whichever ran
            if not cands:
                continue
            k0 = max(cands, key=lambda k: per[k].get("launches", 0) * per[k].get("blobs_per_launch", 0))
            insts = per[k0]["valu_wave_insts_per_blob"]
            achieved_ns = kms[fam] * 1e6 * N_SIMD / (insts * n)
            d[f"{key}_frac_of_mix_floor"] = round(mix[k0]["mix_floor_ns"] / achieved_ns, 4)
            d[f"{key}_wave_insts_per_blob"] = round(insts, 1)
        if rows_per_blob:
            d["rows_per_blob"] = round(rows_per_blob)
            d["rows_per_s"] = round(rows_per_blob * rate)
            d["gather_frac"] = round(rows_per_blob * rate * 128 / 1427.0e9, 4)        # profiles/r03/gather_rate_random_128B.txt: 11.1 G rows/s = 1427 GB/s
        legs[op] = d
    s.free()
    return legs


# What the driver's record of the line keeps: the first ~20 SCALARS of `config`, `roofline` and `cpu_baseline`, in insertion order; nested objects and extra
# top-level keys are dropped.  So the three objects are REBUILT in priority order just before the line is printed: north_star's own
# numbers first, low-value scalars (minima, units, notes, shapes a reader can derive) under a nested `detail`, everything else behind.
CONFIG_PRIORITY_N1 = [
    "workload", "batch_size", "batches_per_step", "inputs",
    "single_call_ms", "single_call_ms_device_hash", "single_call_host_threads", "host_stream_blobs_per_s", "latency_ms_single_batch",
    "commit_blobs_per_s", "commit_msm_bits", "commit_g1_sweep_hbm_frac", "commit_traffic_over_algorithmic", "commit_gather_frac",
    "proof_blobs_per_s", "proof_g1_sweep_hbm_frac", "sclk_mhz_median",
    "commit_default_blobs_per_s", "commit_default_table_gb", "mixed_verify_blobs_per_s", "mixed_commit_blobs_per_s",
    # ... and what no longer fits the kept 20, most useful first
    "proof_traffic_over_algorithmic", "proof_gather_frac", "mid_size_blobs_per_s", "mid_size_one_set_blobs_per_s", "single_call_blobs_per_s", "host_stream_h2d_gbps",
    "verify_kzg_proof_many_per_s", "skipped_for_time", "socket_power_w_median", "commit_table_gb", "commit_msm_frac_of_mix_floor", "proof_quotient_ms",
    "proof_quotient_frac_of_mix_floor"]
CONFIG_PRIORITY_MULTI = [
    "workload", "batch_size", "batches_per_step", "inputs", "value_exchange",
    "allgather_blobs_per_s", "allgather_split_blobs_per_s", "alltoall_blobs_per_s", "parity_gate",
    "stage1_ms_allgather", "exchange_ms_allgather", "stage2_ms_allgather", "merge_ms_allgather", "exchange_ms_alltoall", "stage2_ms_allgather_split",
    "in_library_single_call_ms", "in_library_blobs_per_s", "in_library_exchange", "skipped_for_time", "sclk_mhz_median", "rehearsal",
    "allgather_ms_per_step", "allgather_split_ms_per_step", "alltoall_ms_per_step", "latency_ms_single_batch", "in_library_error"]
CONFIG_DETAIL = ["blobs_per_step", "field_elements_per_blob", "sets_in_flight", "msm_form", "latency_ms_single_batch_min", "single_call_ms_min", "commit_ms_per_launch",
                 "proof_ms_per_launch", "commit_blobs_per_launch", "parity_gate_blobs", "parity_gate_r", "parity_gate_against", "in_library_note",
                 "in_library_single_call_ms_min", "in_library_devices", "in_library_load_s", "in_library_single_call_blobs", "in_library_many_batches"]
ROOFLINE_PRIORITY = ["bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "algorithmic_bytes_per_launch",
                     "path_frac_of_hbm_peak", "alu_path_frac_of_nominal", "alu_path_frac_of_mix_floor", "challenge_ms", "eval_ms", "validate_ms", "lincomb_ms", "pairing_ms",
                     "measured_stream_copy_gbps", "path_bytes_per_blob", "alu_path_wave_insts_per_blob", "lincomb_horner_ms", "launches"]
ROOFLINE_DETAIL = ["traffic_unit", "traffic_source", "kernel_timing", "note"]
CPU_PRIORITY = ["value", "unit", "cores", "kind", "sample", "threads_matched_value", "threads_matched_threads", "all_cores_value", "all_cores_threads", "primitives",
                "portable_c_value", "host_cpus", "cpu_model"]


def _is_scalar(v):
    return v is None or isinstance(v, (bool, int, float, str))


def reorder(d, priority, detail=()):
    """`d` rebuilt: the priority keys that are present (scalars) first, in that order; then the remaining scalars as they were; `detail` keys moved into a nested
    "detail" object; nested objects last.  Nothing is lost -- readers of the raw line find every key; the driver's truncated record finds the right ones."""
    out = {}
    for k in priority:
        if k in d and _is_scalar(d[k]):
            out[k] = d[k]
    det = {k: d[k] for k in detail if k in d and k not in out}
    for k, v in d.items():
        if k not in out and k not in det and _is_scalar(v):
            out[k] = v
    if det:
        out["detail"] = det
    for k, v in d.items():
        if k not in out and k not in det:
            out[k] = v
    return out


def flatten_scalars(line, host_inputs, mid_size, power, msm_legs, coexist=None, multi=False):
    """Every number BASELINE.md quotes becomes a flat scalar of config / roofline / cpu_baseline, then the three objects are put in the order the driver's
    record needs (see CONFIG_PRIORITY_* above; tests/test_bench_launcher.py asserts the first twenty).  The nested objects stay for readers of the raw line."""
    cfg, roof, cpu = line["config"], line.get("roofline"), line.get("cpu_baseline")
    if host_inputs:
        cfg["single_call_ms"] = host_inputs["single_call_ms"]                      # ONE verify_blob_kzg_proof_batch(n = 64) on host slices (benches/kzg_benches.rs:113-120)
        cfg["single_call_ms_min"] = host_inputs["single_call_ms_min"]
        cfg["single_call_blobs_per_s"] = host_inputs["single_call_blobs_per_s"]
        cfg["single_call_ms_device_hash"] = host_inputs["single_call_ms_device_hash"]
        cfg["single_call_host_threads"] = host_inputs.get("single_call_host_threads")      # host threads that hashed for that call (the handle's workers + the caller)
        cfg["host_stream_blobs_per_s"] = host_inputs["stream_blobs_per_s"]         # pageable host memory -> HBM inside the call
        cfg["host_stream_h2d_gbps"] = host_inputs["stream_h2d_gbps"]
    if mid_size:
        cfg["mid_size_blobs_per_s"] = mid_size["blobs_per_s"]                      # 1024-batch sets (8.6 GB), three in flight
        cfg["mid_size_one_set_blobs_per_s"] = mid_size["blobs_per_s_one_set_at_a_time"]
    if power:
        cfg["sclk_mhz_median"] = power["sclk_mhz"]["median"]
        cfg["socket_power_w_median"] = power["socket_power_w"]["median"]
    if msm_legs:
        for op in ("commit", "proof"):
            d = msm_legs[op]
            cfg[f"{op}_blobs_per_s"] = d["blobs_per_s"]
            cfg[f"{op}_ms_per_launch"] = d["ms_per_launch"]
            cfg[f"{op}_g1_sweep_hbm_frac"] = d["g1_sweep_hbm_frac"]
            cfg[f"{op}_traffic_over_algorithmic"] = d["traffic_over_algorithmic"]
            cfg[f"{op}_gather_frac"] = d.get("gather_frac")
        cfg["commit_msm_bits"] = msm_legs["msm_bits"]
        cfg["commit_table_gb"] = msm_legs["table_gb"]
        cfg["commit_blobs_per_launch"] = msm_legs["blobs_per_launch"]
        cfg["proof_quotient_ms"] = msm_legs["proof"]["kernel_ms"].get("quotient")
        cfg["commit_msm_frac_of_mix_floor"] = msm_legs["commit"].get("msm_frac_of_mix_floor")
        cfg["proof_quotient_frac_of_mix_floor"] = msm_legs["proof"].get("quotient_frac_of_mix_floor")
        cfg["msm_legs"] = msm_legs
    if coexist:
        # the table a DEFAULT handle sizes for itself and verification + commitments served by ONE handle with nothing freed in between
        cfg["commit_default_blobs_per_s"] = coexist.get("commit_default_blobs_per_s")
        cfg["commit_default_table_gb"] = coexist.get("commit_default_table_gb")
        cfg["mixed_verify_blobs_per_s"] = coexist.get("mixed_verify_blobs_per_s")
        cfg["mixed_commit_blobs_per_s"] = coexist.get("mixed_commit_blobs_per_s")
        cfg["coexistence"] = coexist
    if roof:
        per = roof.get("per_kernel") or {}
        for fam, key in (("eval", "eval"), ("challenge", "challenge"), ("validate_points", "validate"), ("lincomb", "lincomb"), ("pairing", "pairing"),
                         ("lincomb_horner", "lincomb_horner"), ("rpowers", "rpowers")):
            if fam in per:
                roof[f"{key}_ms"] = per[fam]["avg_launch_ms"]
                roof[f"{key}_frac"] = per[fam]["frac"]
        alu = roof.get("alu") or {}
        if "path_frac_of_nominal" in alu:
            roof["alu_path_frac_of_nominal"] = alu["path_frac_of_nominal"]
            roof["alu_path_wave_insts_per_blob"] = alu["path_valu_wave_insts_per_blob"]
        if "path_frac_of_mix_floor" in alu:
            roof["alu_path_frac_of_mix_floor"] = alu["path_frac_of_mix_floor"]
        for fam, d in (alu.get("per_kernel") or {}).items():
            if "frac_of_mix_floor" in d:
                roof[f"alu_{fam}_frac_of_mix_floor"] = d["frac_of_mix_floor"]
            roof[f"alu_{fam}_frac_of_nominal"] = d["frac_of_nominal"]
        line["roofline"] = reorder(roof, ROOFLINE_PRIORITY, ROOFLINE_DETAIL)
    if cpu:
        if cpu.get("all_cores"):
            cpu["all_cores_value"] = cpu["all_cores"]["value"]
            cpu["all_cores_threads"] = cpu["all_cores"]["threads"]
        line["cpu_baseline"] = reorder(cpu, CPU_PRIORITY)
    line["config"] = reorder(cfg, CONFIG_PRIORITY_MULTI if multi else CONFIG_PRIORITY_N1, CONFIG_DETAIL)


def stream_copy_peak(torch, dev):
    """Measured device-to-device stream copy on this box (read + write bytes per second), reported next to the 8 TB/s nominal."""
    n = 1 << 30
    try:
        a = torch.empty(n, dtype=torch.uint8, device=dev); b = torch.empty_like(a)
        a.random_(0, 255)
        for _ in range(2):
            b.copy_(a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        reps = 10
        for _ in range(reps):
            b.copy_(a)
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        del a, b
        return round(2 * n * reps / (ms / 1e3) / 1e9, 1)
    except Exception:
        return None


def host_leg(L, s, t_blobs, commitments, proofs, n_local, groups):
    """The reference-shaped measurements (benches/kzg_benches.rs:97-122 times the whole call on host slices): blobs in pageable
    host memory, through the drop-in C ABI, H2D inside the call.  (a) one verify_blob_kzg_proof_batch(n = 64) call alone;
    (b) `groups` batches streamed by one kzg355_verify_blob_kzg_proof_batch_many call (chunked H2D / kernel pipeline inside the library)."""
    nb = groups * n_local
    h = t_blobs[:nb * BLOB].cpu().numpy()
    hp = h.ctypes.data_as(C.c_char_p)
    ok1 = C.c_bool()

    def single_calls(reps):
        ts = []
        for i in range(reps + 2):
            t0 = time.perf_counter()
            rc = L.kzg355_verify_blob_kzg_proof_batch(C.byref(ok1), hp, n_local, commitments[:48 * n_local], n_local, proofs[:48 * n_local], n_local, s.handle)
            ts.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0 and ok1.value
        return ts[2:]
    before = s.host_hashed_calls
    lat = single_calls(15)                                        # the library's default route: challenges hashed on the host for a call of this size
    hashed_on_host = s.host_hashed_calls - before >= 15           # every timed call took the host route
    s.set_host_hash(-1)                                           # -1: the per-blob challenges AND the batch challenge r stay on the device
    lat_dev = single_calls(7)                                     # the same call with both device hashes forced (A/B of the host route)
    s.set_host_hash(0)
    okg = (C.c_bool * groups)(); stg = (C.c_int * groups)()
    rates = []
    for i in range(4):
        t0 = time.perf_counter()
        rc = L.kzg355_verify_blob_kzg_proof_batch_many(okg, stg, hp, commitments[:48 * nb], proofs[:48 * nb], n_local, groups, s.handle)
        dt = time.perf_counter() - t0
        assert rc == 0 and all(okg[i] for i in range(groups))
        if i:
            rates.append(nb / dt)
    best = max(rates)
    return {"single_call_ms": round(statistics.median(lat), 3), "single_call_ms_min": round(min(lat), 3),
            "single_call_blobs_per_s": round(n_local / (statistics.median(lat) / 1e3), 1),
            "single_call_host_threads": s.host_threads if hashed_on_host else 1,
            "single_call_route": "Fiat-Shamir challenges and the batch challenge hashed on host threads while the copies and point kernels run" if hashed_on_host else "device hash",
            "single_call_ms_device_hash": round(statistics.median(lat_dev), 3),
            "stream_blobs_per_s": round(statistics.median(rates), 1), "stream_blobs_per_s_best": round(best, 1),
            "stream_h2d_gbps": round(statistics.median(rates) * (BLOB + 96) / 1e9, 2), "stream_blobs_per_call": nb,
            "note": "pageable caller memory -> HBM inside the call (the runtime locks the caller's pages and DMAs from them, 1 GiB chunks over 3 streams); never `value`.  "
                    "single_call = one verify_blob_kzg_proof_batch(n = 64) on host slices, the reference bench's own shape (benches/kzg_benches.rs:113-120)"}


def coexist_leg(L, s, t_blobs, t_c, t_p, commitments, n_local, n_commit, g=1024, rounds=6):
    """ONE default handle serving both paths with everything resident (the verify step's 69 GB of blobs, the table the handle sized for itself):
      * commit_default: kzg355_blob_to_kzg_commitment_many_device over n_commit blobs per launch on the DEFAULT table (a handle left to itself takes the
        widest form that fits half of the free HBM: 15-bit windows, 68.9 GB on an empty card; config.commit_* further down is the explicit 16-bit / 143.5 GB form);
      * mixed: `rounds` times a 1024-batch verify launch set, then an n_commit-blob commitment launch, alternating on the same handle without freeing
        anything; each kind's rate over the time spent in its own calls, and the combined wall.  Reference: blob_to_kzg_commitment (kzg.rs:401-406) and
        verify_blob_kzg_proof_batch (kzg.rs:637-693) take the same &KzgSettings."""
    bits, wins, glv, table_bytes = s.msm_shape()
    out48 = C.create_string_buffer(48 * n_commit)
    st = (C.c_int * n_commit)()
    ok = (C.c_bool * g)(); stg = (C.c_int * g)()

    def commit():
        rc = L.kzg355_blob_to_kzg_commitment_many_device(out48, st, t_blobs.data_ptr(), n_commit, s.handle)
        assert rc == 0 and out48.raw[:48 * n_commit] == commitments[:48 * n_commit]

    def verify():
        rc = L.kzg355_verify_blob_kzg_proof_batch_many_device(ok, stg, t_blobs.data_ptr(), t_c.data_ptr(), t_p.data_ptr(), n_local, g, s.handle)
        assert rc == 0 and bytes(ok)[:g] == b"\x01" * g

    commit(); commit()
    t0 = time.perf_counter()
    for _ in range(4):
        commit()
    default_rate = 4 * n_commit / (time.perf_counter() - t0)
    verify(); commit()
    tv = tc = 0.0
    t_all = time.perf_counter()
    for _ in range(rounds):
        t0 = time.perf_counter(); verify(); tv += time.perf_counter() - t0
        t0 = time.perf_counter(); commit(); tc += time.perf_counter() - t0
    wall = time.perf_counter() - t_all
    return {"commit_default_blobs_per_s": round(default_rate, 1), "commit_default_msm_bits": bits, "commit_default_table_gb": round(table_bytes / 1e9, 1),
            "commit_default_blobs_per_launch": n_commit,
            "mixed_verify_blobs_per_s": round(rounds * g * n_local / tv, 1), "mixed_commit_blobs_per_s": round(rounds * n_commit / tc, 1),
            "mixed_rounds": rounds, "mixed_verify_batches_per_set": g, "mixed_wall_s": round(wall, 3),
            "mixed_share_of_wall_verify": round(tv / wall, 3),
            "note": "one default handle, nothing freed between the calls: the verify step's inputs and workspaces (~80 GB) stay resident beside the handle's own "
                    "table; verify sets of 1024 batches and commitment launches alternate from one host thread"}


def mid_size_leg(L, s, t_blobs, t_c, t_p, n_local, g=1024, depth=3, steps=24):
    """What a caller gets WITHOUT 69 GB resident per call: launch sets of 1024 batches (8.6 GB of blobs), three kept in flight by one host thread
    through kzg355_verify_blob_kzg_proof_batch_many_device_submit / kzg355_verify_collect (stage 2 of a set runs beside the evaluation and point
    kernels of the next one), next to the same sets one at a time through the synchronous call.  Reported in config.mid_size_sets; never `value`."""
    slots = [((C.c_bool * g)(), (C.c_int * g)()) for _ in range(depth)]

    def run(d, n_steps):
        pending, free = [], list(slots)
        t0 = time.perf_counter()
        for _ in range(n_steps):
            if d == 1:
                ok, st = free[0]
                rc = L.kzg355_verify_blob_kzg_proof_batch_many_device(ok, st, t_blobs.data_ptr(), t_c.data_ptr(), t_p.data_ptr(), n_local, g, s.handle)
                assert rc == 0 and bytes(ok)[:g] == b"\x01" * g
                continue
            tk = C.c_void_p()
            rc = L.kzg355_verify_blob_kzg_proof_batch_many_device_submit(C.byref(tk), t_blobs.data_ptr(), t_c.data_ptr(), t_p.data_ptr(), n_local, g, s.handle)
            assert rc == 0, rc
            pending.append((tk, free.pop()))
            if len(pending) >= d:
                tk0, slot = pending.pop(0)
                assert L.kzg355_verify_collect(tk0, slot[0], slot[1]) == 0 and bytes(slot[0])[:g] == b"\x01" * g
                free.append(slot)
        while pending:
            tk0, slot = pending.pop(0)
            assert L.kzg355_verify_collect(tk0, slot[0], slot[1]) == 0 and bytes(slot[0])[:g] == b"\x01" * g
            free.append(slot)
        return n_steps * g * n_local / (time.perf_counter() - t0)
    run(1, 3); run(depth, 6)
    one = run(1, steps)
    piped = run(depth, steps)
    return {"batches_per_set": g, "sets_in_flight": depth, "blobs_per_s": round(piped, 1), "blobs_per_s_one_set_at_a_time": round(one, 1), "steps": steps,
            "note": "device-resident, 1024-batch launch sets (8.6 GB of blobs each) submitted and collected by one host thread; profiles/r04/pipeline_sweep.txt"}


def newest_profile(stem, key, tag=None):
    """newest committed profiles/rNN/<stem>[_tag]_vK.json that has one of `key` in its per_kernel map (numeric round / version order).  tag:
    the summary of that bench op (`commit` / `proof`: their MSM kernels run at another launch size and table width than the ones in the verify
    bench's untimed setup); None: the untagged (verify) summary.  Falls back to any summary that has the kernel."""
    def version(f):
        m = re.search(r"r(\d+)[/\\]" + stem + r"(?:_(\w+?))?_v(\d+)\.json$", f)
        if not m:
            return (0, 0, 0)
        return (1 if (m.group(2) or None) == tag else 0, int(m.group(1)), int(m.group(3)))
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", stem + "_*.json")), key=version, reverse=True):
        try:
            per = json.load(open(f))["per_kernel"]
        except Exception:
            continue
        if any(k in per for k in key):
            return f, per
    return None, None


def pmc_traffic(kernel_family, blobs_per_launch, tag=None):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 --pmc passes (FETCH_SIZE doubled per
    MI355X_MICROARCH.md, WRITE_SIZE as is; separate passes, collected with this same bench command).  The counters are per
    blob there; scaled to this run's launch size.  None if no summary is committed for that kernel."""
    if kernel_family not in KERNEL_NAMES:
        return None, None
    f, per = newest_profile("pmc_traffic", KERNEL_NAMES[kernel_family], tag)
    if not f:
        return None, None
    ds = [per[k] for k in KERNEL_NAMES[kernel_family] if k in per]
    if kernel_family in ALTERNATIVE_FORMS:
        ds = ds[:1]
    per_blob = sum(d["fetch_bytes_per_blob_x2_corrected"] + d["write_bytes_per_blob"] for d in ds)
    return per_blob * blobs_per_launch, os.path.relpath(f, ROOT)


def alu_roofline(stats, blobs_per_launch_of, blobs_per_s_per_gpu, insts_scale_of=lambda fam: 1.0):
    """The bound that binds: VALU issue.  Wave-instructions per blob of every kernel family come from the committed SQ counter
    pass (profiles/rNN/sq_*_vK.json, tools/sq_summary.py: SQ_INSTS_VALU at the bench's launch size); the durations are this
    run's live HIP-event averages.  Fractions are quoted against the NOMINAL issue peak (1024 SIMDs x 2.4 GHz / 2 cycles per
    wave64 instruction); the measured issue rates of the instruction classes involved (profiles/rNN/valu_ceiling.json, from
    tools/ubench/valu_rates.hip: most integer VOP3 / 64-bit instructions issue at half rate) ride along as context."""
    out = {"nominal_peak_wave_insts_per_s": NOMINAL_WAVE_INSTS_PER_S, "per_kernel": {}, "source": None}
    ceil_files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "valu_ceiling.json")))
    ceiling = json.load(open(ceil_files[-1])) if ceil_files else None
    total_insts = 0.0
    # the floor of each kernel's OWN instruction mix at the measured class rates (tools/inst_mix.py: static full-rate / half-rate counts from the
    # gfx950 disassembly of the shipped objects x 1.12 / 1.78 ns per wave-instruction per SIMD, profiles/r02/valu_issue_rates.txt)
    mix_files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "inst_mix.json")))
    mix = json.load(open(mix_files[-1]))["per_kernel"] if mix_files else {}
    floor_ns_weighted = 0.0
    for fam, (tot_ms, cnt) in stats.items():
        names = KERNEL_NAMES.get(fam)
        if not names:
            continue
        f, per = newest_profile("sq", names)
        if not f:
            continue
        ds = [per[k] for k in names if k in per]
        if fam in ALTERNATIVE_FORMS:
            ds = ds[:1]
        insts = sum(d["valu_wave_insts_per_blob"] for d in ds) * insts_scale_of(fam)
        wait = ds[0].get("wait_inst_any_frac")
        rate = insts * blobs_per_launch_of(fam) / (tot_ms / cnt / 1e3)
        total_insts += insts
        out["per_kernel"][fam] = {"valu_wave_insts_per_blob": round(insts, 1), "achieved_wave_insts_per_s": rate,
                                  "frac_of_nominal": round(rate / NOMINAL_WAVE_INSTS_PER_S, 4), "wait_inst_any_frac": wait}
        # instruction-weighted floor over the kernels of the family that ran (SQ counts as weights)
        fl = [(d["valu_wave_insts_per_blob"], mix[k]["mix_floor_ns"]) for k, d in ((k, per[k]) for k in names if k in per) if k in mix]
        if fam in ALTERNATIVE_FORMS:
            fl = fl[:1]
        if fl and rate:
            floor_ns = sum(w * f for w, f in fl) / sum(w for w, _ in fl)
            achieved_ns = N_SIMD / rate * 1e9
            out["per_kernel"][fam].update({"mix_floor_ns_per_wave_inst_per_simd": round(floor_ns, 4), "achieved_ns_per_wave_inst_per_simd": round(achieved_ns, 4),
                                           "frac_of_mix_floor": round(floor_ns / achieved_ns, 4)})
            floor_ns_weighted += floor_ns * insts
        out["source"] = os.path.relpath(f, ROOT)
    if total_insts:
        out["path_valu_wave_insts_per_blob"] = round(total_insts, 1)
        out["path_achieved_wave_insts_per_s"] = total_insts * blobs_per_s_per_gpu
        out["path_frac_of_nominal"] = round(total_insts * blobs_per_s_per_gpu / NOMINAL_WAVE_INSTS_PER_S, 4)
        out["nominal_ceiling_blobs_per_s"] = round(NOMINAL_WAVE_INSTS_PER_S / total_insts, 1)
        if floor_ns_weighted:
            # the step if every kernel issued at the floor of its own mix: sum(insts x floor_ns) / 1024 SIMDs per blob
            out["mix_floor_source"] = os.path.relpath(mix_files[-1], ROOT)
            out["mix_floor_ceiling_blobs_per_s"] = round(N_SIMD * 1e9 / floor_ns_weighted, 1)
            out["path_frac_of_mix_floor"] = round(blobs_per_s_per_gpu / (N_SIMD * 1e9 / floor_ns_weighted), 4)
    if ceiling:
        # context only, not a bound: measured issue rates of the instruction classes this path is made of (tools/ubench/valu_rates.hip).  Round 2
        # quoted kernel rates against "ceilings" derived from these and got fractions above 1: the ubench bodies are two loop bodies of this
        # code, not a limit of the hardware.  The roofline figure is frac_of_nominal.
        out["measured_issue_rates"] = {k: ceiling[k] for k in ("source", "note", "ns_per_wave_inst_per_simd") if k in ceiling}
    return out


def run_sweep(args, kz, L, s, dev, random_blob):
    """benches/kzg_benches.rs:46-126 restated: the five single-op benches and verify_blob_kzg_proof_batch/{1,...,64}, each a
    single call on host buffers through the drop-in C ABI (criterion's iter_batched_ref shape: inputs built outside the timed
    call), median and min over repeated calls, next to the CPU port (oracle, 1 thread) on the same inputs."""
    from oracle.oracle import Oracle, build
    n_max = 64
    blobs = [random_blob(i) for i in range(n_max)]
    B = [kz.Blob(b) for b in blobs]
    cs = kz.Kzg.blob_to_kzg_commitment_many(B, s)
    ps = kz.Kzg.compute_blob_kzg_proof_many(B, cs, s)
    cb, pb = [c.to_bytes() for c in cs], [p.to_bytes() for p in ps]
    z = bytes(31) + b"\x05"
    try:
        build(native=True); o = Oracle(native=True)
    except Exception:
        o = Oracle(native=False)
    golden = os.path.join(ROOT, "tests", "golden")
    so = o.load_trusted_setup(open(os.path.join(golden, "trusted_setup_g1.bin"), "rb").read(), open(os.path.join(golden, "trusted_setup_g2.bin"), "rb").read())

    def timeit(fn, reps, warm=2):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4)}

    proof0, y0 = kz.Kzg.compute_kzg_proof(B[0], kz.Bytes32(z), s)
    gpu_ops = {
        "blob_to_kzg_commitment": lambda: kz.Kzg.blob_to_kzg_commitment(B[0], s),
        "compute_kzg_proof": lambda: kz.Kzg.compute_kzg_proof(B[0], kz.Bytes32(z), s),
        "compute_blob_kzg_proof": lambda: kz.Kzg.compute_blob_kzg_proof(B[0], cs[0], s),
        "verify_kzg_proof": lambda: kz.Kzg.verify_kzg_proof(cs[0], kz.Bytes32(z), y0, proof0, s),
        "verify_blob_kzg_proof": lambda: kz.Kzg.verify_blob_kzg_proof(B[0], cs[0], ps[0], s),
    }
    cpu_ops = {
        "blob_to_kzg_commitment": lambda: o.blob_to_kzg_commitment(blobs[0], so),
        "compute_kzg_proof": lambda: o.compute_kzg_proof(blobs[0], z, so),
        "compute_blob_kzg_proof": lambda: o.compute_blob_kzg_proof(blobs[0], cb[0], so),
        "verify_kzg_proof": lambda: o.verify_kzg_proof(cb[0], z, y0.to_bytes(), proof0.to_bytes(), so),
        "verify_blob_kzg_proof": lambda: o.verify_blob_kzg_proof(blobs[0], cb[0], pb[0], so),
    }
    single = {}
    for name in gpu_ops:
        assert gpu_ops[name]() is not False
        single[name] = {"gpu": timeit(gpu_ops[name], 15), "cpu_port_1_thread": timeit(cpu_ops[name], 5, warm=1)}
    # the *_many forms of the single-proof functions (one verify_kzg_proof per call is a 1.9 ms latency-bound chain on a GPU; the reference's
    # bench shape, benches/kzg_benches.rs:58-91, has no batched counterpart): units per second of ONE call over many units, next to the CPU port's per-call rate
    zs = [kz.Bytes32(bytes(31) + bytes([5 + i])) for i in range(n_max)]
    pys = kz.Kzg.compute_kzg_proof_many(B, zs, s)
    n_checks = 16384
    reps = n_checks // n_max
    cm = b"".join(cb) * reps; zm = b"".join(z_.to_bytes() for z_ in zs) * reps
    ym = b"".join(y_.to_bytes() for _, y_ in pys) * reps; pm = b"".join(p_.to_bytes() for p_, _ in pys) * reps
    okm = (C.c_bool * n_checks)(); stm = (C.c_int * n_checks)()

    def many_verify():
        rc = L.kzg355_verify_kzg_proof_many(okm, stm, cm, zm, ym, pm, n_checks, s.handle)
        assert rc == 0 and bytes(okm) == b"\x01" * n_checks
    n_units = 1024                                                # blob forms: the 64 blobs tiled to 1024 units (128 MiB of host memory per call)
    tile = n_units // n_max
    flat_all = b"".join(blobs) * tile
    cflat, pflat = b"".join(cb) * tile, b"".join(pb) * tile
    okb = (C.c_bool * n_units)(); stb = (C.c_int * n_units)()
    outp = C.create_string_buffer(48 * n_units); outy = C.create_string_buffer(32 * n_units)
    zflat = b"".join(z_.to_bytes() for z_ in zs) * tile
    want_p = b"".join(p_.to_bytes() for p_, _ in pys) * tile

    def many_verify_blob():
        rc = L.kzg355_verify_blob_kzg_proof_many(okb, stb, flat_all, cflat, pflat, n_units, s.handle)
        assert rc == 0 and bytes(okb) == b"\x01" * n_units

    def many_compute():
        rc = L.kzg355_compute_kzg_proof_many(outp, outy, stb, flat_all, zflat, n_units, s.handle)
        assert rc == 0 and outp.raw == want_p
    many = {}
    for name, fn, units, cpu_name in (("verify_kzg_proof_many", many_verify, n_checks, "verify_kzg_proof"), ("verify_blob_kzg_proof_many", many_verify_blob, n_units, "verify_blob_kzg_proof"),
                                      ("compute_kzg_proof_many", many_compute, n_units, "compute_kzg_proof")):
        g = timeit(fn, 7)
        cpu_ms = single[cpu_name]["cpu_port_1_thread"]["median_ms"]
        many[name] = {"units_per_call": units, "gpu": dict(g, units_per_s=round(units / (g["median_ms"] / 1e3), 1)),
                      "cpu_port_1_thread_units_per_s": round(1e3 / cpu_ms, 1), "gpu_single_call_units_per_s": round(1e3 / single[cpu_name]["gpu"]["median_ms"], 1)}
    sweep = {}
    flat = b"".join(blobs)
    ok1 = C.c_bool()
    for n in (1, 2, 4, 8, 16, 32, 64):
        cc, pp = b"".join(cb[:n]), b"".join(pb[:n])

        def gpu_call():
            rc = L.kzg355_verify_blob_kzg_proof_batch(C.byref(ok1), flat, n, cc, n, pp, n, s.handle)
            assert rc == 0 and ok1.value
        g = timeit(gpu_call, 15)
        c = timeit(lambda: o.verify_blob_kzg_proof_batch(blobs[:n], cb[:n], pb[:n], so), 3 if n >= 16 else 5, warm=1)
        sweep[str(n)] = {"gpu": dict(g, blobs_per_s=round(n / (g["median_ms"] / 1e3), 1)),
                         "cpu_port_1_thread": dict(c, blobs_per_s=round(n / (c["median_ms"] / 1e3), 1))}
    o.free_trusted_setup(so)
    g64 = sweep["64"]["gpu"]
    return {"metric": OP_METRIC["verify"] + " -- criterion sweep, single calls on host inputs", "value": g64["blobs_per_s"], "unit": "blobs/s",
            "n_gpus": 1, "steps": 15, "warmup": 2, "ms_per_step": g64["median_ms"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u32 limbs (29-bit) / 64-bit accumulate, u8 bytes", "data": "synthetic",
            "config": {"workload": "benches/kzg_benches.rs:46-126: five single-op benches + verify_blob_kzg_proof_batch/{1,2,4,8,16,32,64}, one call at a time, host buffers",
                       "verify_kzg_proof_many_per_s": many["verify_kzg_proof_many"]["gpu"]["units_per_s"],
                       "verify_kzg_proof_cpu_port_per_s": many["verify_kzg_proof_many"]["cpu_port_1_thread_units_per_s"],
                       "verify_blob_kzg_proof_many_per_s": many["verify_blob_kzg_proof_many"]["gpu"]["units_per_s"],
                       "compute_kzg_proof_many_per_s": many["compute_kzg_proof_many"]["gpu"]["units_per_s"],
                       "single_op": single, "many_forms": many, "verify_blob_kzg_proof_batch": sweep},
            "roofline": None, "cpu_baseline": {"value": sweep["64"]["cpu_port_1_thread"]["blobs_per_s"], "unit": "blobs/s", "cores": 1, "kind": "port",
                                               "sample": "per-n / per-op figures under config; oracle -O3 -march=native, restatement in portable C, not blst"}}


def cpu_model():
    """the host CPU's model name ("print nproc, CPU model" next to the CPU baseline)"""
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.lower().startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def time_cpu_baseline(op, commitments, proofs, host_blobs, n, match_threads=None, all_threads=True):
    """The CPU oracle (kind "port": the build's restatement of the reference algorithm, NOT blst) on the host cores of
    this box: verify_blob_kzg_proof_batch over the same first 64-blob batch, single thread like the reference."""
    from oracle.oracle import Oracle, build
    try:
        build(native=True)
        o = Oracle(native=True)
    except Exception:
        o = Oracle(native=False)
    golden = os.path.join(ROOT, "tests", "golden")
    so = o.load_trusted_setup(open(os.path.join(golden, "trusted_setup_g1.bin"), "rb").read(),
                              open(os.path.join(golden, "trusted_setup_g2.bin"), "rb").read())
    blobs = [bytes(host_blobs[i * BLOB:(i + 1) * BLOB]) for i in range(n)]
    cs = [commitments[48 * i:48 * i + 48] for i in range(n)]
    ps = [proofs[48 * i:48 * i + 48] for i in range(n)]
    def one_core(seconds):
        reps, t_total, units = 0, 0.0, 0
        while t_total < seconds and reps < 200:
            t0 = time.perf_counter()
            if op == "verify":
                assert o.verify_blob_kzg_proof_batch(blobs, cs, ps, so) is True
                units += n
            elif op == "commit":
                assert o.blob_to_kzg_commitment(blobs[reps % n], so) == cs[reps % n]
                units += 1
            else:
                assert o.compute_blob_kzg_proof(blobs[reps % n], cs[reps % n], so) == ps[reps % n]
                units += 1
            t_total += time.perf_counter() - t0
            reps += 1
        return reps, t_total, units
    # Two forms of the port's hot primitives (oracle/bls12_381.c): portable C (__int128 products, C SHA-256) and -- when the -march=native build found
    # BMI2 + ADX (+ SHA) on this host -- mulx / adcx / adox Montgomery products with SHA-extension hashing, the instruction mix of blst's assembly.
    # `value` is the faster one: the stronger baseline is the honest one to quote.
    fast = bool(getattr(o, "has_fast_primitives", False))
    portable = None
    if fast:
        o.set_fast_primitives(False)
        r0, t0_, u0 = one_core(5.0)
        portable = u0 / t0_
        o.set_fast_primitives(True)
    reps, t_total, units = one_core(10.0)
    # the stronger baseline SURVEY 8(d) asks for: every core of this box's share, one batch (or blob) per thread
    # (ctypes releases the GIL; the oracle holds no mutable state in its settings)
    import threading
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    avail = max(1, cores)

    def run_threads(cores):
        done = [0] * cores
        t_end = time.perf_counter() + 5.0
        def worker(k):
            j = k
            while time.perf_counter() < t_end:
                if op == "verify":
                    o.verify_blob_kzg_proof_batch(blobs, cs, ps, so); done[k] += n
                elif op == "commit":
                    o.blob_to_kzg_commitment(blobs[j % n], so); done[k] += 1
                else:
                    o.compute_blob_kzg_proof(blobs[j % n], cs[j % n], so); done[k] += 1
                j += cores
        t0 = time.perf_counter()
        th = [threading.Thread(target=worker, args=(k,)) for k in range(cores)]
        for t in th: t.start()
        for t in th: t.join()
        return sum(done) / (time.perf_counter() - t0)
    # the box's CPUs are shared with the other GPUs' jobs: try its per-GPU share and every CPU this process may run on, keep the better
    trials = {c: run_threads(c) for c in sorted({min(avail, 64), avail})} if all_threads else {}
    cores = max(trials, key=trials.get) if trials else None
    all_cores = trials[cores] if trials else None
    # the reference-shaped single call (config.single_call_ms) hashes on config.single_call_host_threads host threads beside the GPU; the CPU
    # figure to hold against it is the port on AS MANY threads (one batch per thread), not one core
    matched = None
    if match_threads and match_threads > 1:
        k = min(int(match_threads), avail)
        matched = {"value": trials[k] if k in trials else run_threads(k), "threads": k}
    o.free_trusted_setup(so)
    what = {"verify": "verify_blob_kzg_proof_batch(n=64) on the bench's first batch", "commit": "blob_to_kzg_commitment on blobs of the first batch",
            "proof": "compute_blob_kzg_proof on blobs of the first batch"}[op]
    return {"value": units / t_total, "unit": "blobs/s", "cores": 1, "kind": "port",
            "sample": f"{reps} x {what}, oracle -O3 -march=native, {t_total:.1f} s; the builder's restatement of the reference's algorithm, not blst"
                      + (": Montgomery products with mulx / adcx / adox, SHA-256 with the SHA extensions (the portable-C form of the same code: portable_c_value)" if fast else
                         " (portable C: this host has no BMI2 + ADX; blst's asm is likely 1.5-3x faster per core)"),
            "primitives": "mulx/adcx/adox + sha-ni" if fast else "portable C", "portable_c_value": portable,
            "host_cpus": os.cpu_count(), "cpu_model": cpu_model(),
            "threads_matched_value": matched["value"] if matched else None, "threads_matched_threads": matched["threads"] if matched else None,
            "all_cores": {"value": all_cores, "threads": cores, "cpus_available": avail, "trials": {str(k): round(v, 1) for k, v in trials.items()},
                          "note": "same work, one call per thread, ~5 s per trial; best of the trials"} if trials else None}


if __name__ == "__main__":
    main()
