"""Headline benchmark: Swin-T + 8-layer decoder greedy decode, 128 tokens, batches of 64
384x384x1 images per GPU (BASELINE.json configs[1]; configs[2] when run with N ranks).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A step = encode + 128-step greedy decode of one 64-image batch (images resident in HBM),
then, with N > 1 ranks, an RCCL all-gather of the decoded token streams inside
libmathocr.so (``mocr_group_gather_ids``; image-parallel shards, no other collective;
torch.distributed over gloo carries only the group id, barriers and the timing max).

Each engine call takes G = --chain-batches batches of 64 (default ``auto_chain``: the largest
G <= 10 that makes the timed batches a whole number of calls per replica -- 8 at the default
64 steps, 10 at the driver's 20): one encode of the G*64 images and ONE decode chain of
G*64 rows.  A greedy step is a chain of 41 dependent
kernels whose launch and memory latencies do not grow with the rows, so G batches in one
chain amortise them G ways (profiles/r03/decode_chain_probe_*.log); rows are
independent (stop="none" here; tests/test_gpu_parity.py::test_wide_chain_rows_bitwise
holds a row's logits bitwise equal between a 2-row and a 160-row chain).  Each GPU
pipelines calls through R engine replicas (``pipeline.ReplicaPool``, one host thread and
one HIP stream each), so one call's decode overlaps the next call's encoder.  Rank 0
prints one JSON line; ``value`` = all images all ranks processed / max-over-ranks time.

``--cu-split`` (off by default, for A/B runs) gives each replica its own equal share of
the device's compute units (``isolate_replicas``); docs/replica_nondeterminism.md has the
finding it served.

A plain run sets up, warms up, times exactly ``--steps`` batches, writes its outputs when
``--dump-outputs DIR`` is given and prints the line.  ``--full`` adds the passes that take
runs of their own: the 16-call latency pass (``p50_image_latency_ms``), the single-replica
latency / roofline pass, the literal config-2 pass and the CPU baseline (each still
switched off by its ``--no-...`` option).  When the timed batches are no whole number of
equal calls, ``call_plan`` splits them into calls that differ by one batch, so ``steps``
in the line is always the ``--steps`` asked for.

``--dump-outputs DIR`` writes, after the timed region, what the timed path returned to its
caller: the token ids ``[rows, tokens + 1]`` of each replica's last full call, as float32 in
``DIR/ids_rank<r>_replica<i>.npy`` (of its last call of the plan's largest size: where the
calls are unequal, which replica gets the smaller ones is up to the pool, and a smaller
batch can take other kernels), and the
encoder memory ``[32, M, 256]`` that call's decode read for 32 images evenly spaced over
its rows, in
``DIR/memory_rank<r>_replica<i>.npy`` (a float array to compare within a tolerance: one
changed token changes every token after it).  Each
replica decodes its own seeded images on every call, so the files depend only on the
arguments, never on which replica the pool gave the last call to.

``--gpus N`` (N > 1) without a launcher (no WORLD_SIZE in the environment) starts
``torch.distributed.run --nproc-per-node N`` on this file as a child process, before
anything touches the GPU, and exits with its status; under a launcher, --gpus must equal
WORLD_SIZE.  The line's ``rccl_ranks`` is what RCCL's communicator counts
(``mocr_group_size`` = ncclCommCount), null when the ranks share one device and gather
over the host group.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import socket
import statistics
import subprocess
import sys
import time

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

METRIC = "images/sec + p50 per-image latency, Swin-T+8L-dec greedy@128tok, 1/2/4/8 GPU"
# dense peaks (MI355X_MICROARCH.md): MFMA TFLOP/s by operand type, HBM GB/s
PEAK = {"f32": 157.3, "bf16": 2500.0, "bf16x3": 2500.0}
HBM_PEAK_GBS = 8000.0
DTYPE = {"fp32": "f32", "bf16x3": "bf16x3", "bf16": "bf16"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64,
                    help="timed batches per GPU (the replica pipeline's fill and drain are inside the timed "
                         "region: 64 batches read 0.8 %% above 24, profiles/r02/bench_steps_probe.log)")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=64, help="images per batch (per GPU)")
    ap.add_argument("--image", type=int, nargs=2, default=[384, 384])
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3", "bf16"])
    ap.add_argument("--replicas", type=int, default=None,
                    help="engine replicas pipelining calls per GPU (default: 2 with 4-batch chains, 4 with 1)")
    ap.add_argument("--chain-batches", dest="chain", type=int, default=None,
                    help="64-image batches per engine call / decode chain (default: auto_chain, 4 or 5; 1 for "
                         "res18trans, whose encoder attends across its batch, and for beam search)")
    ap.add_argument("--full", action="store_true", default=False,
                    help="also run what the headline figure does not need: the 16-call latency pass, the "
                         "single-replica latency / roofline pass, the literal config-2 pass, the CPU baseline")
    ap.add_argument("--dump-outputs", dest="dump_outputs", default=None, metavar="DIR",
                    help="after the timed steps, write each replica's last token ids and a 32-image sample of "
                         "its encoder memory to DIR/<name>.npy (float32)")
    ap.add_argument("--cu-split", dest="cu_split", action="store_true", default=False,
                    help="A/B: each replica on its own share of the compute units instead of all of them "
                         "(isolate_replicas; docs/replica_nondeterminism.md)")
    ap.add_argument("--no-secondary", dest="secondary", action="store_false", default=True,
                    help="skip the literal config-2 pass (64 images per engine call, 4 replicas)")
    ap.add_argument("--cpu-baseline", dest="cpu_baseline", action="store_true", default=True)
    ap.add_argument("--no-cpu-baseline", dest="cpu_baseline", action="store_false")
    ap.add_argument("--cpu-sample", type=int, default=64,
                    help="images per CPU-baseline throughput run (BASELINE.md §3: B = 64, median of 3)")
    ap.add_argument("--cpu-runs", type=int, default=3)
    ap.add_argument("--no-isolated", dest="isolated", action="store_false", default=True,
                    help="skip the single-replica latency / roofline pass")
    ap.add_argument("--arch", default="swin", choices=["swin", "res18trans"],
                    help="res18trans: BASELINE config 5 (src/model_res18trans.py)")
    ap.add_argument("--beam", type=int, default=0,
                    help="K > 0: beam search (BASELINE config 4: --beam 4 --batch 32 --tokens 256)")
    ap.add_argument("--variant", default="",
                    help="comma-separated engine.VARIANT names (A/B of a kernel path; empty = production)")
    ap.add_argument("--lib", default=None,
                    help="an in-tree A/B build of libmathocr.so (tools/build_variant.sh) instead of lib/")
    a = ap.parse_args()
    if a.beam and a.arch != "swin":
        ap.error("--beam is measured on the Swin path")
    if a.gpus < 1:
        ap.error("--gpus must be >= 1")
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if a.chain is not None and a.chain > 1 and (a.arch != "swin" or a.beam):
        ap.error("--chain-batches > 1 is for the Swin greedy path (the ResNet18-trans encoder attends across its batch)")
    if a.replicas is None:
        a.replicas = 2 if (a.chain is None or a.chain > 1) and a.arch == "swin" and not a.beam else 4
    a.chain_auto = a.chain is None
    if a.chain is None:
        a.chain = 1 if (a.arch != "swin" or a.beam) else auto_chain(a.steps, a.replicas)
    return a


def auto_chain(steps, replicas, g_max=10):
    """Batches of 64 per engine call: the largest G <= g_max that splits the timed batches
    into a whole number of calls per replica.  More images in flight raise throughput (a
    decode step's 41 dependent launches cost little more at 512-640 rows than at 256, and
    two concurrent chains overlap their latencies) at the cost of the call's latency: on one
    box, 64 batches at 4 / 8 x 64 with 2 replicas gave 4410 / 4798-4889 img/s at p50 114 /
    209-213 ms; 20 batches at 5 / 10 x 64 gave 4302 / 4807 img/s at p50 148 / 266 ms; four
    replicas or 16 x 64 saturate near 4900 (profiles/r04/r04e-f).  Uneven calls per replica
    leave the last call's decode chain alone at the end of the timed region."""
    for g in range(g_max, 3, -1):
        if steps % g == 0 and (steps // g) % replicas == 0:
            return g
    return 4


def call_plan(steps, chain, replicas, auto, g_max=10):
    """Batches of 64 in each timed engine call, in call order; they sum to ``steps``.  Equal
    calls of ``chain`` batches where that divides the steps.  Otherwise calls that differ by
    one batch, the larger first: as few as hold at most ``chain`` batches each, or, when the
    chain length was left to the benchmark (``auto``), the smallest multiple of the replicas
    that holds at most ``g_max`` each (13 steps on 2 replicas: 7 + 6)."""
    if steps % chain == 0:
        return [chain] * (steps // chain)
    if auto:
        calls = min(steps, replicas * -(-steps // (g_max * replicas)))
    else:
        calls = -(-steps // chain)
    q, r = divmod(steps, calls)
    return [q + 1] * r + [q] * (calls - r)


def isolate_replicas(pool, n_cu, sharers=1, slot=0):
    """Give every engine of the pool its own contiguous range of the device's compute units
    (``Engine.set_cu_mask``): the device's CUs split evenly over ``sharers`` processes on it
    (this one the ``slot``-th) times the pool's replicas.  ``--cu-split`` only: the A/B
    arrangement that located the finding in docs/replica_nondeterminism.md.  Returns the
    ranges as [first, last + 1] per engine; no split (None) for a single engine alone."""
    parts = sharers * len(pool.engines)
    if parts < 2:
        return None
    span = n_cu // parts
    if span < 1:
        raise SystemExit(f"bench.py: {parts} engines on a device of {n_cu} compute units")
    out = []
    for i, e in enumerate(pool.engines):
        first = (slot * len(pool.engines) + i) * span
        e.set_cu_mask(range(first, first + span))
        out.append([first, first + span])
    return out


MEMORY_DUMP_ROWS = 32  # images whose encoder memory --dump-outputs keeps (4.7 MB each replica)


def dump_outputs(out_dir, rank, ids_per_replica, rows, memories=()):
    """``--dump-outputs``: the first ``rows`` rows of the token ids of each replica's last
    full-size call, [rows, tokens + 1], as float32 (ids < 2^24 are exact) in
    ``out_dir/ids_rank<rank>_replica<i>.npy``, and beside them ``memories[i]``, the encoder
    memory [n <= MEMORY_DUMP_ROWS, M, 256] of a fixed sample of that call's images, in
    ``memory_rank<rank>_replica<i>.npy``."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for i, ids in enumerate(ids_per_replica):
        np.save(os.path.join(out_dir, f"ids_rank{rank}_replica{i}.npy"), ids[:rows].cpu().numpy().astype(np.float32))
    for i, mem in enumerate(memories):
        if len(mem) > MEMORY_DUMP_ROWS:
            raise ValueError(f"dump_outputs: {len(mem)} memory rows, at most {MEMORY_DUMP_ROWS} are kept")
        np.save(os.path.join(out_dir, f"memory_rank{rank}_replica{i}.npy"), np.asarray(mem, dtype=np.float32))


def warm_replicas(pool, step, items=(0,)):
    """One untimed call on EVERY replica, each engine driven directly (``pool.imap`` gives an
    item to whichever replica is free, so a short warm-up may never reach one): each
    engine's first decode of this (rows, steps, stop) captures and instantiates its 16 graph
    chunks (engine.hip graph_for), which must not land in the timed region.
    ``items``: one call per entry on each engine (the call sizes the timed region holds).
    Returns the engines warmed, in order."""
    warmed = []
    for e in pool.engines:
        for it in items:
            step(e, it)
        warmed.append(e)
    return warmed


class stdout_to_stderr:
    """Route file descriptor 1 to 2 for the block: gloo's connect messages ("[Gloo] Rank r is
    connected to ...") are written to the process's stdout by the C++ library, and the
    driver reads rank 0's stdout as the ONE JSON line of the run."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)
        return False


def free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launcher_cmd(n, argv, port):
    """The torch.distributed.run command that runs this file on n local ranks."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
            "--master-addr=127.0.0.1", f"--master-port={port}", os.path.abspath(__file__), *argv]


def launch_if_needed(args, argv, env=None):
    """--gpus N > 1 without a launcher: run N ranks under torch.distributed.run as a child
    process (never exec: the parent has not touched the GPU, but the child must own it)
    and return its exit status; None when this process is a rank (or N = 1).  Under a
    launcher, WORLD_SIZE must equal --gpus."""
    env = os.environ if env is None else env
    world = env.get("WORLD_SIZE")
    if world is not None:
        if int(world) != args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: pass --gpus equal to the "
                             f"launcher's --nproc-per-node")
        return None
    if args.gpus == 1:
        return None
    return subprocess.run(launcher_cmd(args.gpus, argv, free_port())).returncode


def cpu_threads():
    """torch.set_num_threads(len(os.sched_getaffinity(0))), capped by
    OMP_NUM_THREADS where the box sets it (the GPU box's CPU share is smaller than the
    machine the affinity mask shows)."""
    n = len(os.sched_getaffinity(0))
    cap = os.environ.get("OMP_NUM_THREADS")
    if cap and cap.isdigit() and int(cap) > 0:
        n = min(n, int(cap))
    return n


def cpu_baseline(args, pkg):
    """The oracle restatement of the reference CPU path (src/inference.py: full-prefix
    re-decode, fp32, torch CPU) on a bounded sample of the same workload:
    one warm-up, then the median of 3 runs at B=1 (latency) and at B=cpu_sample
    (throughput), same seeded images and weights as the GPU run."""
    import platform
    from oracle import model_ref
    threads = cpu_threads()
    torch.set_num_threads(threads)
    w = pkg.synth.make_weights(1234, "init")
    model = model_ref.build_model(w)
    n = args.cpu_sample
    imgs = torch.from_numpy(pkg.synth.make_images(n, *args.image, seed0=1000))
    model_ref.greedy_decode(model, images=imgs[:1], max_steps=2, stop="none")  # warm-up

    def timed(batch):
        t0 = time.perf_counter()
        model_ref.greedy_decode(model, images=imgs[:batch], max_steps=args.tokens, stop="none")
        return time.perf_counter() - t0

    lat = statistics.median(timed(1) for _ in range(args.cpu_runs))
    thr = statistics.median(timed(n) for _ in range(args.cpu_runs))
    cpu = platform.processor() or platform.machine()
    try:
        cpu = next(ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name"))
    except (OSError, StopIteration):
        pass
    return {"value": n / thr, "unit": "images/sec", "cores": threads, "kind": "port",
            "b1_latency_ms": lat * 1e3, "cpu": cpu,
            "sample": f"median of {args.cpu_runs} runs of {n} images (and of 1 image for b1_latency_ms), {args.image[0]}x"
                      f"{args.image[1]}, {args.tokens} greedy steps, full-prefix re-decode as src/inference.py, "
                      f"fp32 torch CPU, {threads} threads; {n}-image run {thr:.1f} s"}


def pmc_traffic(precision, cls, batch):
    """HBM bytes per launch of a kernel class from the committed rocprofv3 PMC passes of
    an encode of `batch` images and 8 greedy steps over them
    (profiles/pmc_traffic_<precision>_b<batch>.json, written by tools/pmc_traffic.py:
    FETCH_SIZE x2 + WRITE_SIZE), or None when no profile of that batch exists (bytes per
    launch depend on the batch)."""
    path = os.path.join(REPO, "profiles", f"pmc_traffic_{precision}_b{batch}.json")
    try:
        return json.load(open(path))["classes"][cls]["hbm_bytes_per_launch"]
    except (OSError, KeyError, ValueError):
        return None


def serving_latency(pkg, weights, precision, device, runs=10):
    """The reference's serving call, one request alone: ``im2latex.predict`` on one 96x320
    image (app/src/im2latex.py:15-55, called from app/src/main.py:486: batch-global stop,
    150-step cap, confidence from the log-probs; the host image copied to the device inside
    the call), and the same image decoded for a fixed 128 steps (encode + decode, images
    resident).  Median of ``runs`` after two warm-up calls.  The reference quotes "~150 ms
    on GPU" per image (README.md:87)."""
    eng = pkg.Engine(img_hw=(96, 320), max_batch=1, precision=precision, device=device)
    eng.load_weights(weights)
    vocab, idx2char = pkg.synth.synthetic_vocab()
    img = pkg.synth.make_images(1, 96, 320, seed0=1000)
    t_pred, t_fix = [], []
    for i in range(runs + 2):
        t0 = time.perf_counter()
        pkg.im2latex.predict(eng, img, vocab, idx2char)
        t1 = time.perf_counter()
        eng.encode(img)
        res = eng.decode(max_steps=128, stop="none")
        t2 = time.perf_counter()
        if i >= 2:
            t_pred.append(t1 - t0)
            t_fix.append(t2 - t1)
    eng.encode(img)
    n_pred = eng.decode(max_steps=pkg.config.config.max_seq_len, stop="batch").n_steps
    eng.close()
    return {"im2latex_predict": statistics.median(t_pred) * 1e3, "im2latex_predict_steps": n_pred,
            "fixed_128_steps": statistics.median(t_fix) * 1e3, "fixed_steps": res.n_steps, "samples": runs,
            "image": [96, 320], "batch": 1, "precision": precision,
            "reference_quote": "~150 ms on GPU per image (README.md:87)"}


# per 384² image 26.39 GFLOP of encoder work at the dense bf16 MFMA peak
# plus 245 MB of bf16 decode traffic at 8 TB/s
E2E_ROOFLINE_IMG_S = 1.0 / (26.39e9 / 2.5e15 + 245e6 / 8e12)


def roofline(stats, dtype, precision, batch, attention=False):
    """Dominant encoder GEMM class (attention=False) or window-attention class
    (attention=True: the fused norm1 + qkv + W-MSA kernels, s3.attn at 384²) by
    event-timed GPU time: algorithmic FLOP per launch / average launch duration, against
    the dense bf16 MFMA peak (fp32 MFMA in fp32 mode).  bf16x3 issues three bf16 MFMAs per
    product (hi*hi + hi*lo + lo*hi), so the MFMA issue rate is 3x the algorithmic rate:
    reported beside it as mfma_issue_frac.  peak_basis says which peak frac divides by
    (round 1 divided bf16x3 by 2500/3; rounds 2-3 by 2500)."""
    gemms = {k: v for k, v in stats.items()
             if v["flops"] > 0 and ("attn" in k) == attention and not k.endswith("stem") and k != "r.enc"
             and not k.startswith("decode")}
    if not gemms:
        return None
    name, d = max(gemms.items(), key=lambda kv: kv[1]["total_ms"])
    avg_ms = d["total_ms"] / d["launches"]
    flops = d["flops"] / d["launches"]
    achieved = flops / (avg_ms * 1e-3) / 1e12
    peak = PEAK[dtype]
    kind = "attention" if attention else f"gemm_{'f32' if dtype == 'f32' else 'bf16'}"
    out = {"kernel": f"{kind}[{dtype}] {name}", "bound": "mfma",
           "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
           "peak_basis": "dense fp32 MFMA" if dtype == "f32" else "dense bf16 MFMA (2.5 PF)",
           "traffic": pmc_traffic(precision, name, batch),
           "avg_launch_ms": avg_ms, "flops_per_launch": flops,
           "algorithmic_bytes_per_launch": d["bytes"] / d["launches"]}
    if dtype == "bf16x3":
        out["mfma_issue_frac"] = 3 * achieved / peak
    return out


def survey_decode_step_bytes(rows, t, L=8, d=256, ff=512, V=5075, M=144):
    """SURVEY.md §8(d)'s algorithmic bytes of one greedy step over `rows` rows, bf16: every
    decoder weight and fc_out once, the cross-attention K/V of all layers, the
    self-attention K/V of positions 0..t read and t written."""
    weights = L * (6 * d * d + 2 * d * ff) + V * d
    return 2.0 * (weights + rows * M * 2 * d * L + rows * (t + 2) * 2 * d * L)


# the greedy steps the committed PMC passes of the decode cover (tools/pmc_traffic.py: an
# encode and 8 greedy steps, t = 0..7): `traffic` is compared with the algorithmic bytes of
# these same steps, not with the t = 0..127 average
PMC_DECODE_STEPS = range(8)


def roofline_decode(stats, precision, rows, steps):
    """The greedy decode step (41 graph-captured dependent kernels) against HBM: SURVEY
    §8(d)'s algorithmic bytes of a step (bf16 K/V and weights) / the HIP-event step time,
    with the engine's as-built bytes (engine.hip decode_step_bytes: fp32 weights or their
    bf16x3 planes, int16 K/V in bf16x3 engines) beside them.  ``traffic`` (PMC, steps 0..7)
    is set against ``algorithmic_bytes_pmc_steps``, the §8(d) bytes of the same steps."""
    d = stats.get("decode.greedy")
    if not d or not d["launches"]:
        return None
    step_ms = d["total_ms"] / d["launches"]
    built = d["bytes"] / d["launches"]
    survey = sum(survey_decode_step_bytes(rows, t) for t in range(steps)) / steps
    pmc_basis = sum(survey_decode_step_bytes(rows, t) for t in PMC_DECODE_STEPS) / len(PMC_DECODE_STEPS)
    traffic = pmc_traffic(precision, "decode.step", rows)
    achieved = survey / (step_ms * 1e-3) / 1e9
    return {"kernel": f"greedy decode step over {rows} rows (8 layers x 5 folded kernels + logits; the selection "
                      f"runs in the next step's first kernel)", "bound": "hbm",
            "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic, "avg_step_ms": step_ms, "rows": rows,
            "algorithmic_bytes_per_step": survey, "bytes_basis": "SURVEY.md §8(d): bf16 weights and K/V",
            "traffic_steps": f"t = {PMC_DECODE_STEPS.start}..{PMC_DECODE_STEPS.stop - 1} (the PMC passes' steps)",
            "algorithmic_bytes_pmc_steps": pmc_basis,
            "traffic_ratio": traffic / pmc_basis if traffic else None,
            "as_built_bytes_per_step": built, "as_built_achieved": built / (step_ms * 1e-3) / 1e9,
            "as_built_frac": built / (step_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "tflops": d["flops"] / d["launches"] / (step_ms * 1e-3) / 1e12}


def main():
    args = parse()
    rc = launch_if_needed(args, sys.argv[1:])
    if rc is not None:
        sys.exit(rc)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = max(1, torch.cuda.device_count())  # counting devices does not initialise the GPU
    shared = int(os.environ.get("LOCAL_WORLD_SIZE", "1")) > ndev  # ranks share a device (1-GPU test box)
    local = local % ndev
    dev = f"cuda:{local}"
    pkg = importlib.import_module("handwritten-math-ocr-api_amd")
    if args.lib:
        pkg.engine.load_library(args.lib, ab_build=True)
    grp = None
    gather = "none"
    rccl_ranks = None
    if world > 1:
        torch.cuda.set_device(local)
        with stdout_to_stderr():
            dist.init_process_group("gloo")  # host-side control only
            dist.barrier()  # every rank connected (gloo prints as it connects)
        if shared:
            # RCCL refuses two ranks on one device: the 33 KB token streams go over the host
            # group instead (only on a box with fewer GPUs than ranks; tests/test_gpu_sharded.py)
            gather = "gloo host (ranks share a device)"
        else:
            gather = "rccl (mocr_group_gather_ids)"
    H, W = args.image
    B, S, R = args.batch, args.tokens, args.replicas
    plan = call_plan(args.steps, args.chain, R, args.chain_auto)  # batches per timed engine call
    G = max(plan)
    BG = B * G  # images per engine call (one encode, one decode chain of BG rows)
    dtype = DTYPE[args.precision]
    calls = len(plan)
    wcalls = -(-args.warmup // G)

    # 256 beam-search tokens need a positional table of >= 257 rows (the reference's has 150,
    # src/model_swin.py:54): synthetic weights with 260 rows for that config
    max_pos = max(pkg.synth.MAX_POS, S + 4) if args.beam else pkg.synth.MAX_POS
    variant = tuple(v for v in args.variant.split(",") if v)
    ekw = dict(img_hw=(H, W), max_batch=BG, precision=args.precision, device=local, arch=args.arch,
               max_beam=args.beam, max_pos=max_pos, variant=variant)
    pool = pkg.pipeline.ReplicaPool(R, **ekw)
    if gather.startswith("rccl"):
        # after the engines: their HIP streams take the process's first hardware queues
        # (GPU_MAX_HW_QUEUES = 4), the group's stream and RCCL's own come after them
        with stdout_to_stderr():
            grp = pkg.parallel.RcclGroup(world, rank, local)  # RCCL inside libmathocr.so
        rccl_ranks = grp.size()  # ncclCommCount
        if rccl_ranks != world:
            raise SystemExit(f"RCCL communicator counts {rccl_ranks} ranks, WORLD_SIZE is {world}")
    weights = pkg.synth.make_weights(1234, "init", arch=args.arch, max_pos=max_pos)
    pool.load_weights(weights)
    # ranks that share a device (a box with fewer GPUs than ranks) share its CUs as well
    n_cu = torch.cuda.get_device_properties(local).multi_processor_count
    sharers = -(-int(os.environ.get("LOCAL_WORLD_SIZE", "1")) // ndev)
    slot = int(os.environ.get("LOCAL_RANK", "0")) // ndev
    cu_split = isolate_replicas(pool, n_cu, sharers, slot) if args.cu_split else None
    # each replica holds its own G batches of this rank's shard, resident in HBM
    resident = {}  # engine -> its images on the device; a call of fewer batches takes the first rows
    for i, e in enumerate(pool.engines):
        seed0 = 1000 + (rank * R + i) * BG
        resident[id(e)] = torch.from_numpy(pkg.synth.make_images(BG, H, W, seed0=seed0)).to(dev)
        e.set_images(resident[id(e)])
        if args.arch == "res18trans":
            e.set_encoder_pos(pkg.synth.make_pos_table(5, e.memory_tokens))
    last_ids = {}  # engine -> the ids its latest full-size call returned (--dump-outputs)

    def step(eng, g):
        """One engine call over g batches of B (0: all the engine's resident images)."""
        t0 = time.perf_counter()
        rows = g * B if g else resident[id(eng)].shape[0]
        if eng.batch != rows:
            # another call size of a plan with unequal calls: at most once per replica in the
            # timed region (the larger calls come first), a device-to-device copy
            eng.set_images(resident[id(eng)][:rows])
        ids = torch.empty((eng.batch, S + 1), dtype=torch.int32, device=dev)
        eng.encode()
        if args.beam:
            r = eng.beam_search(beam=args.beam, max_steps=S, stop="none")
            ids.copy_(torch.from_numpy(r.ids))
        else:
            eng.decode_into(ids, max_steps=S, stop="none")
        if rows == resident[id(eng)].shape[0]:
            last_ids[id(eng)] = ids
        return ids, time.perf_counter() - t0

    def run(n, pool=pool):
        """n: a number of full-size calls, or the list of each call's batches."""
        lat = []
        for ids, dt in pool.imap(step, [0] * n if isinstance(n, int) else n):
            # the all-gather of the token streams, in call order: RCCL on device memory, or the
            # host group when ranks share a device; through the pad-and-trim gather any shard
            # split takes (call k holds the same rows on every rank, so it is one plain gather)
            rows = ids.shape[0]
            if grp:
                pkg.parallel.gather_shards(ids, world * rows, world, rank, grp.gather_ids)
            elif world > 1:
                pkg.parallel.gather_shards(ids.cpu(), world * rows, world, rank,
                                           lambda t: pkg.parallel.gather_ids_host(t, world))
            lat.append(dt)
        return lat

    # every call size of the plan on every replica, the largest last (the pooled warm-up and
    # the first timed calls are of that size)
    sizes = sorted(set(plan))
    warm_replicas(pool, step, sizes)
    run(wcalls)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lat = run(plan)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:
        # of each replica's last full-size call (every replica ran one: the warm-up ends on
        # that size), so which replica the pool gave the plan's smaller calls to, and the
        # kernels a smaller batch takes, change nothing here.  The memory is what that
        # call's decode read; an engine whose last call was smaller encodes its full
        # images once more for it, outside the timed region
        pick = [k * BG // MEMORY_DUMP_ROWS for k in range(MEMORY_DUMP_ROWS)] if BG > MEMORY_DUMP_ROWS else list(range(BG))
        mems = []
        for e in pool.engines:
            if e.batch != BG:
                e.set_images(resident[id(e)])
                e.encode()
            mems.append(e.memory()[pick])
        dump_outputs(args.dump_outputs, rank, [last_ids[id(e)] for e in pool.engines], BG, mems)
    rank_elapsed = [elapsed]
    if world > 1:
        # every rank's time (an 8-GPU run shows any imbalance); the line's time is the max
        t = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(t, torch.tensor([elapsed], dtype=torch.float64))
        rank_elapsed = [float(x.item()) for x in t]
        elapsed = max(rank_elapsed)

    # the latency half of the metric: at least 16 more loaded calls of the same pipelined
    # configuration (the timed region holds as few as 2 with the driver's --steps 20)
    lat_pass = None
    if args.full:
        lat_pass = run(max(16, 2 * R))

    iso = None
    if rank == 0 and args.full and args.isolated:
        # one replica alone: unloaded call latency + HIP-event kernel timing for the roofline
        e = pool.engines[0]
        if cu_split:
            e.set_cu_mask(None)  # alone on the device: all of its CUs
        e.set_timing(True)
        ts = []
        for _ in range(3):
            _, dt = step(e, 0)
            ts.append(dt)
        stats = e.timing()
        e.set_timing(False)
        e1 = pkg.Engine(**dict(ekw, max_batch=1))
        e1.load_weights(weights)
        e1.set_images(torch.from_numpy(pkg.synth.make_images(1, H, W, seed0=1000)).to(dev))
        if args.arch == "res18trans":
            e1.set_encoder_pos(pkg.synth.make_pos_table(5, e1.memory_tokens))
        t1s = []
        for _ in range(3):
            t1 = time.perf_counter()
            e1.encode()
            if args.beam:
                e1.beam_search(beam=args.beam, max_steps=S, stop="none")
            else:
                e1.decode(max_steps=S, stop="none")
            t1s.append(time.perf_counter() - t1)
        e1.close()
        iso = {"call_latency_ms": statistics.median(ts) * 1e3, "b1_latency_ms": statistics.median(t1s) * 1e3,
               "stats": stats}
        # the host->device copy of one call's images, which the timed region leaves out (the
        # images are resident in HBM): pageable numpy source, and pinned
        host = pkg.synth.make_images(BG, H, W, seed0=1000)
        pinned = torch.from_numpy(host).pin_memory()
        h2d = {"pageable": [], "pinned": []}
        for _ in range(3):
            for kind, src in (("pageable", torch.from_numpy(host)), ("pinned", pinned)):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                src.to(dev, non_blocking=kind == "pinned")
                torch.cuda.synchronize()
                h2d[kind].append(time.perf_counter() - t1)
        iso["h2d_ms"] = {k: statistics.median(v) * 1e3 for k, v in h2d.items()}
        iso["h2d_bytes"] = host.nbytes
        del pinned
        if args.arch == "swin" and not args.beam:
            iso["serving"] = serving_latency(pkg, weights, args.precision, local)

    literal = None
    if rank == 0 and world == 1 and args.full and args.secondary and G > 1:
        # BASELINE config 2 read literally: 64 images per engine call (one 64-row chain), 4
        # replicas, images resident; a shorter pass beside the headline
        pool.close()
        lit_pool = pkg.pipeline.ReplicaPool(4, **dict(ekw, max_batch=B))
        lit_pool.load_weights(weights)
        for i, e in enumerate(lit_pool.engines):
            resident[id(e)] = torch.from_numpy(pkg.synth.make_images(B, H, W, seed0=1000 + i * B)).to(dev)
            e.set_images(resident[id(e)])
        if args.cu_split:
            isolate_replicas(lit_pool, n_cu)
        lit_calls = 32
        warm_replicas(lit_pool, step)
        run(8, lit_pool)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lit_lat = run(lit_calls, lit_pool)
        torch.cuda.synchronize()
        lit_s = time.perf_counter() - t1
        lit_pool.close()
        literal = {"value": B * lit_calls / lit_s, "unit": "images/sec", "batches": lit_calls,
                   "images_per_call": B, "replicas": 4, "ms_per_step": lit_s / lit_calls * 1e3,
                   "p50_call_latency_loaded_ms": statistics.median(lit_lat) * 1e3,
                   "note": "64 images per engine call (one encode of 64, one 64-row decode chain), 4 replicas "
                           "pipelining, 8 untimed warm-up calls"}

    if rank != 0:
        pool.close()
        if grp:
            grp.close()
        if world > 1:
            dist.destroy_process_group()
        return

    steps = sum(plan)  # = --steps
    value = world * B * steps / elapsed
    out = {
        "metric": METRIC,
        "value": value,
        "unit": "images/sec",
        "n_gpus": world,
        "rccl_ranks": rccl_ranks,
        "steps": steps,
        "warmup": wcalls * G + R * sum(sizes),
        "warmup_requested": args.warmup,  # rounded up to whole engine calls of G batches
        "call_batches": plan,  # batches of B in each timed engine call, in call order
        "ms_per_step": elapsed / steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": dtype,
        "data": f"synthetic: U(-1,1) {H}x{W}x1 images (PCG64 seeds 1000+i), random-init weights with the "
                f"reference's init distributions (seed 1234"
                + (f", positional table of {max_pos} rows" if args.beam else "")
                + (", encoder positional table torch seed 5" if args.arch == "res18trans" else "")
                + f"); {S} {'beam-' + str(args.beam) if args.beam else 'greedy'} steps, no early stop",
        "config": {"workload": f"{G} x {B} = {BG} images per engine call (one encode, one {BG}-row decode chain), "
                               f"{R} replicas pipelining, {H}x{W} "
                               f"{'Swin-T' if args.arch == 'swin' else 'ResNet18+8L-enc'} + 8L decoder "
                               f"{'beam' + str(args.beam) if args.beam else 'greedy'}@{S}, per GPU; BASELINE "
                               f"config 2 read literally (64 images per call) is config2_literal",
                   # global_batch / per_gpu_batch: BASELINE's batch unit (64 images per GPU, as
                   # rounds 1-4 reported them); images_per_call: one engine call's
                   # encode + decode chain; images_in_flight: over the replicas
                   "global_batch": world * B, "per_gpu_batch": B, "batch_unit": B,
                   "images_per_call": BG, "images_in_flight": BG * R,
                   "image": [H, W], "max_tokens": S, "vocab": pkg.synth.VOCAB,
                   "decoder_layers": pkg.synth.N_LAYERS, "parallelism": f"image-parallel x{world}", "gather": gather,
                   "replicas_per_gpu": R, "cu_split": cu_split, "batches_per_chain": G, "precision": args.precision,
                   "variant": list(variant), "build": pkg.engine.load_library().mocr_build_tag().decode()},
        "e2e_roofline": {"value": value / world, "unit": "images/sec per GPU", "peak": E2E_ROOFLINE_IMG_S,
                         "frac": value / world / E2E_ROOFLINE_IMG_S,
                         "basis": "BASELINE.md §4: 26.39 GFLOP/img at 2.5 PF + 245 MB/img bf16 decode traffic at 8 TB/s"},
        # an image's latency under the bench's load is its engine call's: the call's G batches
        # complete together
        "p50_call_latency_loaded_ms": statistics.median(lat) * 1e3,
        "latency_samples": len(lat),
        "warmup_calls": {"per_replica_direct": len(sizes), "pooled": wcalls,
                         "note": "every replica runs one untimed call of each call size (graph capture) before "
                                 "the pooled warm-up"},
        "rank_elapsed_s": {"min": min(rank_elapsed), "max": max(rank_elapsed), "all": rank_elapsed},
        "full": args.full,
    }
    if lat_pass:
        out.update({
            "p50_image_latency_ms": statistics.median(lat_pass) * 1e3,
            "p90_image_latency_ms": sorted(lat_pass)[max(0, -(-9 * len(lat_pass) // 10) - 1)] * 1e3,
            "image_latency_samples": len(lat_pass),
            "latency_note": (f"p50_image_latency_ms: the loaded latency of an image's engine call ({G} batch(es) of "
                             f"{B} through encode + decode, {R} replicas pipelining), median of "
                             f"{len(lat_pass)} calls run right after the timed region in the same configuration "
                             f"(p50_call_latency_loaded_ms is the median of the timed region's {len(lat)}); "
                             f"p50_image_latency_b1_ms is one 384x384 image alone (B=1); serving_latency_ms is the "
                             f"reference's serving call (96x320, B=1, im2latex.predict)"),
        })
    if literal:
        out["config2_literal"] = literal
    if iso:
        out["p50_call_latency_unloaded_ms"] = iso["call_latency_ms"]
        out["p50_image_latency_b1_ms"] = iso["b1_latency_ms"]
        if "serving" in iso:
            out["serving_latency_ms"] = iso["serving"]
        h2d = iso["h2d_ms"]["pageable"]
        out["h2d_ms_per_call"] = iso["h2d_ms"]
        out["h2d_note"] = (f"host->device copy of one call's {BG} images ({iso['h2d_bytes'] / 1e6:.0f} MB fp32), "
                           f"outside the timed region; serialised with the calls it would give "
                           f"{B * steps / (elapsed + calls * h2d * 1e-3) * world:.0f} img/s (pageable source)")
        rd = roofline_decode(iso["stats"], args.precision, BG, S)
        rg = roofline(iso["stats"], dtype, args.precision, BG)
        ra = roofline(iso["stats"], dtype, args.precision, BG, attention=True)
        # `roofline` is the dominant kernel class by GPU time (HIP events, one call alone):
        # the decode step when its share is the largest, else the dominant encoder GEMM
        dec_ms = iso["stats"].get("decode.greedy", {}).get("total_ms", 0.0)
        gemm_cls = max(((k, v) for k, v in iso["stats"].items() if not k.startswith(("decode", "host"))),
                       key=lambda kv: kv[1]["total_ms"], default=(None, {"total_ms": 0.0}))
        if rd and dec_ms >= gemm_cls[1]["total_ms"]:
            out["roofline"] = rd
            out["roofline_gemm"] = rg
        else:
            out["roofline"] = rg
            if rd:
                out["roofline_decode"] = rd
        if ra:
            out["roofline_attention"] = ra
        enc_ms = sum(v["total_ms"] for k, v in iso["stats"].items() if not k.startswith(("decode", "host"))) / 3
        out["gpu_time_share"] = {"decode": dec_ms / 3 / (dec_ms / 3 + enc_ms) if dec_ms else 0.0,
                                 "encoder_ms_per_call": enc_ms, "decode_ms_per_call": dec_ms / 3}
        out["encoder_ms_per_batch_events"] = enc_ms / G
        out["kernel_classes"] = {k: {"launches": v["launches"], "avg_ms": v["total_ms"] / v["launches"],
                                     "tflops": v["flops"] / v["total_ms"] * 1e-9 if v["total_ms"] else None}
                                 for k, v in sorted(iso["stats"].items())}
    if args.full and args.cpu_baseline and world == 1 and args.arch == "swin" and not args.beam:
        out["cpu_baseline"] = cpu_baseline(args, pkg)
    if not literal:
        pool.close()
    print(json.dumps(out))
    if grp:
        grp.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
