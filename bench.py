"""Headline benchmark: SlowFast-R50 32x2x224 bf16 training throughput (clips/s, whole job).

    python bench.py --gpus N --steps K --warmup W

``--gpus N > 1`` without a torchrun environment: this process starts
``python -m torch.distributed.run --nproc-per-node N`` as a CHILD (before touching the GPU), waits for it
and exits with its status; each rank then runs one GPU (RCCL over xGMI).  Under torchrun/``accelerate
launch`` (``WORLD_SIZE`` set) it runs as one rank directly.

One training step = on-device video preprocessing of synthetic decoded uint8 clips (temporal subsample,
random short-side scale, random crop, flip, normalise, PackPathway) → fused SlowFast forward/backward
on the gfx950 kernels → bucketed RCCL gradient all-reduce overlapped with backward → fused SGD +
weight re-pack.  Weights are random-init (no network); data is synthetic uint8 frames of the Kinetics
clip shape (64 source frames = 2.13 s at 30 fps, 256x340).  Timing: W untimed warmup steps (plus one
untimed autotuning pass, in which the ranks agree on kernel configurations), then K steps bracketed by
barrier + device synchronize, max over ranks; rank 0 prints one JSON line.  ``ms_per_step`` is the wall time of the
K timed steps divided by K.  A plain run does nothing beyond that; secondary measurements go behind ``--full``.

``--dump-outputs DIR``: after the timed steps rank 0 writes what the last timed step returned — ``loss.npy``,
``logits.npy`` [batch, classes] — and ``params.npy``, a fixed seeded sample of the flat parameters after that step,
all float32 (17 MB at the defaults).  Model, data, augmentation parameters and dropout key are seeded, so the inputs
are the same in every run with the same arguments.  What is computed from them repeats only on the
bitwise-reproducible executor: the default one adds weight gradients with atomics in arrival order and sums split
reductions in an order the autotuner picks, and the random-init network amplifies that rounding noise from step to
step, up to several per cent in the logits after a dozen optimizer steps.  So that two runs, or two builds, can be
compared array for array, ``--dump-outputs`` selects ``--deterministic 1`` unless the caller passes
``--deterministic 0``; a note on stderr and ``config.deterministic`` in the result line say which executor ran.  The
deterministic executor is slower (one stream, generic stems, built-in kernel choices), and ``value`` and
``ms_per_step`` of such a run are that executor's: the headline figure comes from a run without this option.
``--deterministic 0 --dump-outputs DIR`` times and dumps the default executor, with the run-to-run noise above.

``--plumbing``: CPU/gloo rehearsal of the same launch + gradient-sync path on the reference PyTorch
modules (tiny crop, no dropout) — what the CPU test suite drives (tests/test_bench_launch_cpu.py).
Reference launch being benchmarked: ``run_slowfast_r50.sh:1`` / ``run.py:196-198`` (accelerate DDP).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

METRIC = "clips/sec (whole node) SlowFast-R50 32x2x224 at 1/2/4/8 MI355X; step-time p50"
# Stock PyTorch-ROCm eager (MIOpen conv3d + ATen BN + DDP) measured on one MI355X with the same
# model/config/synthetic data (scripts/baseline_torch.py; profiles/baseline_torch/bench.jsonl): 73.1 clips/s
# at B=8, 75.35 at B=32 — the better of the two is the per-GPU baseline (reference publishes none).
STOCK_CLIPS_PER_S_1GPU = 75.35


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0,
                    help="per-GPU clips per step (default 160; 32 for --precision fp32)")
    ap.add_argument("--model", choices=("slowfast", "slow_r50"), default="slowfast",
                    help="slowfast: SlowFast-R{--depth} (headline); slow_r50: Slow-only R50 (the reference run.py default "
                         "model, is_slowfast=False, run.py:338-351), e.g. --model slow_r50 --frames 8")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--alpha", type=int, default=4)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--classes", type=int, default=400)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--src-frames", type=int, default=64)
    ap.add_argument("--src-h", type=int, default=256)
    ap.add_argument("--src-w", type=int, default=340)
    ap.add_argument("--bucket-mb", type=float, default=32.0)
    ap.add_argument("--first-bucket-mb", type=float, default=4.0)
    ap.add_argument("--grad-dtype", choices=("fp32", "bf16"), default="fp32",
                    help="all-reduce payload dtype (bf16 = DDP bf16_compress_hook analogue)")
    ap.add_argument("--precision", choices=("bf16", "fp16", "fp32"), default="bf16",
                    help="bf16/fp16: compute type of the fused kernels (fp16 adds dynamic loss scaling, the reference "
                         "recipe's --mixed_precision fp16, run_slowfast_r50.sh:9); fp32: the native fp32 kernels (the "
                         "reference default --mixed_precision no, run.py:330; models/native32.py)")
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--grad-accum", type=int, default=1,
                    help="micro-batches of --batch clips per optimizer step (gradients all-reduced once, on the last)")
    ap.add_argument("--graph", type=int, default=0,
                    help="1: replay each micro-step (+ SGD) as a captured HIP graph (single process; engine/graph.py)")
    ap.add_argument("--plumbing", action="store_true", help="CPU/gloo rehearsal on the PyTorch modules")
    ap.add_argument("--dump", default=None,
                    help="write the first optimizer step's (all-reduced) flat gradient and every rank's final "
                         "parameters here (cross-rank numerics tests)")
    ap.add_argument("--deterministic", type=int, choices=(0, 1), nargs="?", const=1, default=None,
                    help="1 (or no value): bitwise-reproducible fused executor (fixed-order reductions, one stream; "
                         "cross-rank exactness tests); 0: the default executor.  Default: 0, or 1 with --dump-outputs")
    ap.add_argument("--source", choices=("synthetic", "host"), default="synthetic",
                    help="synthetic: decoded uint8 clips resident on the device (preprocessing only); host: a raw-frame "
                         ".npy corpus read by the native C++ reader into pinned memory, H2D on a copy stream, then "
                         "the same on-device preprocessing (the reference's DataLoader + H2D path, run.py:170-183,243)")
    ap.add_argument("--corpus", default="/tmp/pva_bench_corpus",
                    help="--source host: corpus directory (generated on first use)")
    ap.add_argument("--corpus-videos", type=int, default=96)
    ap.add_argument("--reader-threads", type=int, default=16)
    ap.add_argument("--data-rank", type=int, default=-1,
                    help="draw the synthetic data of this rank instead of the own one (single-process oracle runs "
                         "of a multi-rank job's shards)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step returned (loss, logits) and a fixed "
                         "seeded sample of the parameters it left behind as DIR/<name>.npy, float32.  Selects "
                         "--deterministic 1 unless --deterministic 0 is given (stderr and the result line say so): "
                         "only that executor's outputs repeat from run to run")
    ap.add_argument("--full", action="store_true",
                    help="also run whatever the benchmark measures beyond its headline figure (secondary "
                         "measurements belong here, never in a plain run; there are none at present)")
    a = ap.parse_args(argv)
    if a.deterministic is None:
        # dumped outputs repeat from run to run only on the bitwise-reproducible executor (module docstring)
        a.deterministic = int(bool(a.dump_outputs))
        if a.dump_outputs and not a.plumbing and int(os.environ.get("RANK", "0")) == 0:
            print("bench.py: --dump-outputs runs the deterministic executor (slower; --deterministic 0 keeps the "
                  "default one, whose outputs differ from run to run)", file=sys.stderr)
    a.deterministic = bool(a.deterministic)
    if not a.batch:
        a.batch = 32 if a.precision == "fp32" else 160
    return a


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(a, argv) -> int:
    """Run this script as ``a.gpus`` torchrun ranks in a child process; returns its exit status.

    Called before anything initialises the GPU (``torch.cuda.device_count`` does not), and never via
    exec: the child is a separate process and this one only waits for it."""
    # PVA_DIST_BACKEND=gloo: a 1-GPU rehearsal of the multi-rank path (ranks share the device)
    if not a.plumbing and os.environ.get("PVA_DIST_BACKEND") != "gloo":
        ndev = torch.cuda.device_count()
        if ndev < a.gpus:
            print(f"bench.py: --gpus {a.gpus} requested but only {ndev} GPU(s) visible", file=sys.stderr)
            return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.call(cmd, env=env)


# ---------------------------------------------------------------------------------------------- plumbing
def plumbing_model(a):
    from pytorchvideo_accelerate_amd.models import reference as R
    torch.manual_seed(1234)
    s = a.crop // 32
    return R.create_slowfast(a.depth, a.classes, alpha=a.alpha, dropout_rate=0.0,
                             head_pool_kernel_sizes=((a.frames // a.alpha, s, s), (a.frames, s, s)))


def plumbing_batch(a, rank: int, i: int):
    g = torch.Generator().manual_seed(1000 + 7919 * rank + i)
    fast = torch.randn(a.batch, 3, a.frames, a.crop, a.crop, generator=g)
    idx = torch.linspace(0, a.frames - 1, a.frames // a.alpha).long()
    return [fast.index_select(2, idx).contiguous(), fast], torch.randint(0, a.classes, (a.batch,), generator=g)


# ---------------------------------------------------------------------------------------------- host source
def build_corpus(a, rank: int) -> str:
    """Raw-frame Kinetics-layout corpus (README 'Data'): ``corpus-videos`` uint8 [src_frames, H, W, 3] .npy videos
    at 30 fps over 8 classes, random pixels.  Written once (rank 0; the others wait on a marker file)."""
    import numpy as np
    root = os.path.join(a.corpus, f"{a.src_frames}x{a.src_h}x{a.src_w}_{a.corpus_videos}")
    done = os.path.join(root, ".complete")
    if os.path.exists(done):
        return root
    if rank != 0:
        while not os.path.exists(done):
            time.sleep(0.5)
        return root
    rng = np.random.default_rng(0)
    for i in range(a.corpus_videos):
        d = os.path.join(root, "train", f"class_{i % 8}")
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"v{i:04d}.npy")
        mm = np.lib.format.open_memmap(path + ".tmp.npy", mode="w+", dtype=np.uint8,
                                       shape=(a.src_frames, a.src_h, a.src_w, 3))
        for t in range(a.src_frames):
            mm[t] = rng.integers(0, 256, size=(a.src_h, a.src_w, 3), dtype=np.uint8)
        mm.flush()
        del mm
        os.replace(path + ".tmp.npy", path)
    open(done, "w").close()
    return root


def host_loader(a, st, eng, dev):
    """Endless device batches: VideoClipDataset (random clip, scale, crop, flip per clip; this rank's shard) ->
    NativeRawSource (C++ thread pool preads the 32 kept frames of each clip into pinned memory) -> DeviceLoader
    (H2D of batch i+1 on a copy stream while batch i trains) -> fused on-device preprocessing."""
    from pytorchvideo_accelerate_amd.data.kinetics import LabeledVideoPaths, VideoClipDataset
    from pytorchvideo_accelerate_amd.data.loader import DeviceLoader, NativeRawSource
    from pytorchvideo_accelerate_amd.data.transforms import GpuClipBatch
    root = build_corpus(a, st.rank)
    vids = LabeledVideoPaths.from_directory(os.path.join(root, "train"))
    # repeat the video list so one pass covers every step (each repeat draws fresh random clips / augmentations)
    need = (a.warmup + a.steps + 3) * a.batch * a.grad_accum * st.world_size
    reps = -(-need // max(len(vids), 1))
    paths = LabeledVideoPaths([vids[i] for i in range(len(vids))] * reps, vids.classes)
    alpha = None if a.model == "slow_r50" else a.alpha
    ds = VideoClipDataset(paths, a.src_frames / 30.0, True, a.frames, a.crop, alpha, rank=st.rank,
                          world=st.world_size, distributed=st.world_size > 1, seed=0, mode="gpu")
    src = NativeRawSource(ds, a.batch, threads=a.reader_threads, drop_last=True, prefetch=3)
    prep = GpuClipBatch(dev, a.frames, a.crop, alpha, s2d=eng.input_s2d, dtype=eng.cdt)
    while True:
        for b in DeviceLoader(src, prep, dev):
            yield b["video"], b["label"]


# ---------------------------------------------------------------------------------------------- outputs
OUTPUT_SAMPLE = 4 * 2 ** 20   # elements kept of an output larger than this (16 MiB as float32)


def dump_outputs(root: str, arrays) -> None:
    """``--dump-outputs``: every array as ``root/<name>.npy`` in float32.  An array of more than OUTPUT_SAMPLE
    elements is reduced to that many distinct (flattened) elements, at sorted indices drawn from a fixed seed — the
    same indices in every run and every build, so two dumps compare element for element."""
    import numpy as np
    os.makedirs(root, exist_ok=True)
    for name, t in arrays.items():
        if t is None:
            continue
        t = t.detach()
        if t.numel() > OUTPUT_SAMPLE:
            g = torch.Generator().manual_seed(20240229)
            idx = torch.randperm(t.numel(), generator=g)[:OUTPUT_SAMPLE].sort().values   # each element once
            t = t.reshape(-1).index_select(0, idx.to(t.device))
        np.save(os.path.join(root, name + ".npy"), t.float().cpu().numpy())


# ---------------------------------------------------------------------------------------------- main
def run(a):
    from pytorchvideo_accelerate_amd.parallel.dist import DistState
    from pytorchvideo_accelerate_amd.parallel.ddp import GradSync
    from pytorchvideo_accelerate_amd.ops.optim import FusedSGD
    from pytorchvideo_accelerate_amd.utils.profiling import trace_range

    st = DistState.from_env(cpu=a.plumbing)
    dev = st.device
    gdt = torch.bfloat16 if a.grad_dtype == "bf16" else None
    B = a.batch
    dump = {}
    kept = {}      # logits of the most recent micro-step (--dump-outputs)
    gstep = None   # engine.graph.GraphedStep when --graph 1 (single process)
    scaler = None
    skipped = [0]  # fp16: optimizer steps skipped by the loss scaler (overflow)
    if a.plumbing:
        from pytorchvideo_accelerate_amd.engine.backends import TorchBackend
        be = TorchBackend(plumbing_model(a), st, "no", a.bucket_mb)
        be.sync = GradSync(be.flat.grad, st, a.bucket_mb, first_mb=a.first_bucket_mb, grad_dtype=gdt)
        st.broadcast_tensors([be.flat.data] + list(be.model.buffers()))
        be.train()
        opt = FusedSGD(be.flat, lr=a.lr, momentum=0.9, weight_decay=1e-4)
        sync = be.sync

        def step(i, tune=False):
            opt.zero_grad()
            for j in range(a.grad_accum):
                xs, y = plumbing_batch(a, st.rank, i * a.grad_accum + j)
                loss, kept["logits"] = be.train_step(xs, y, loss_scale=1.0 / a.grad_accum, sync=j == a.grad_accum - 1)
            if i == 0 and a.dump:
                dump["grad"] = be.flat.grad.clone()
            opt.step()
            return loss
    else:
        from pytorchvideo_accelerate_amd.models import reference as R
        from pytorchvideo_accelerate_amd.models.fused import FusedNet
        from pytorchvideo_accelerate_amd.data.transforms import GpuClipBatch, sample_params
        assert dev.type == "cuda", "bench.py needs a GPU (or --plumbing)"
        torch.manual_seed(1234)
        slow_only = a.model == "slow_r50"
        model = (R.create_resnet(50, a.classes, head_pool_kernel_size=(a.frames, a.crop // 32, a.crop // 32))
                 if slow_only else R.create_slowfast(a.depth, a.classes))
        alpha = None if slow_only else a.alpha
    if not a.plumbing and a.precision == "fp32":
        from pytorchvideo_accelerate_amd.models.native32 import NativeF32Net
        assert a.source == "synthetic" and not a.graph, "--precision fp32 runs synthetic device clips, eagerly"
        eng = NativeF32Net(model, dev)
        st.broadcast_tensors([eng.flat.data] + [b for b in model.buffers()])
        opt = FusedSGD(eng.flat, lr=a.lr, momentum=0.9, weight_decay=1e-4)
        bounds = sorted(set(eng.flat.span(p)[1] for p in eng.flat.params))
        sync = GradSync(eng.flat.grad, st, a.bucket_mb, boundaries=bounds, first_mb=a.first_bucket_mb,
                        grad_dtype=gdt, timing=st.multi)
        eng.grad_hook = sync.progress if st.multi else None
        sync.producers = lambda: [torch.cuda.current_stream(dev)]
        drank = st.rank if a.data_rank < 0 else a.data_rank
        gen = torch.Generator().manual_seed(1000 + drank)
        labels_all = torch.randint(0, a.classes, (64, B), generator=gen).to(dev)
        # synthetic normalised clips already on the device (what the host transform + H2D deliver), two batches
        # alternated; the NCTHW -> NDHWC layout pass runs inside every step
        clips = []
        for _ in range(2):
            fast = torch.randn(B, 3, a.frames, a.crop, a.crop, generator=gen).to(dev)
            clips.append(fast if slow_only else
                         [fast[:, :, torch.linspace(0, a.frames - 1, a.frames // a.alpha).long()].contiguous(), fast])

        def step(i, tune=False):
            opt.zero_grad()
            for j in range(a.grad_accum):
                k = i * a.grad_accum + j
                last = j == a.grad_accum - 1
                sync.begin(last and not tune)
                loss, kept["logits"] = eng.forward_backward(clips[k % 2], labels_all[k % 64],
                                                            loss_scale=1.0 / a.grad_accum)
                sync.finish()
            if tune:
                return None
            with trace_range("sgd"):
                opt.step()
            return loss
    elif not a.plumbing:
        from pytorchvideo_accelerate_amd.ops.optim import FusedGradScaler
        assert not (a.graph and a.precision == "fp16"), "--graph replays no loss-scale check"
        eng = FusedNet(model, dev, deterministic=a.deterministic, load_tuning=st.world_size == 1,
                       compute_dtype=torch.float16 if a.precision == "fp16" else torch.bfloat16)
        scaler = FusedGradScaler() if a.precision == "fp16" else None
        if st.multi:
            eng.tuner.agree = st.agree_times
            ts = eng.tune_store   # rank 0's persistent autotuner table, broadcast once (as engine/backends.py)
            doc = st.broadcast_object(ts.read() if (ts is not None and st.rank == 0) else None)
            if ts is not None:
                ts.restore(doc)
                ts.writer = st.rank == 0
        st.broadcast_tensors([eng.flat.data] + [b for b in model.buffers()])
        eng.pack()
        opt = FusedSGD(eng.flat, lr=a.lr, momentum=0.9, weight_decay=1e-4, after_step=eng.pack)
        bounds = sorted(set(eng.flat.span(p)[1] for p in eng.flat.params))
        sync = GradSync(eng.flat.grad, st, a.bucket_mb, boundaries=bounds, first_mb=a.first_bucket_mb,
                        grad_dtype=gdt, timing=st.multi)
        eng.grad_hook = sync.progress if st.multi else None   # (1 GPU: no buckets to launch)
        sync.producers = eng.producer_streams   # RCCL: buckets issued from the sync's own comm stream
        eng.grad_multi_stream = sync.multi_stream
        drank = st.rank if a.data_rank < 0 else a.data_rank
        gen = torch.Generator().manual_seed(1000 + drank)
        labels_all = torch.randint(0, a.classes, (64, B), generator=gen).to(dev)
        host_labels = [None]
        if a.source == "host":
            assert not a.graph, "--source host replays no graph (fresh input buffers every step)"
            hl = host_loader(a, st, eng, dev)

            def batch(k):
                xs, lab = next(hl)
                host_labels[0] = lab
                return xs
        else:
            frames = torch.empty(B, a.src_frames, a.src_h, a.src_w, 3, dtype=torch.uint8, device=dev)
            eng.C.synth_frames(frames, 7 + drank)
            # double-buffered on-device preprocessing: micro-batch k+1 is decoded/resized/cropped on its own
            # stream while micro-batch k trains (a prefetching data loader; every step still pays its batch)
            preps = [GpuClipBatch(dev, a.frames, a.crop, alpha, s2d=eng.input_s2d, dtype=eng.cdt) for _ in range(2)]
            pstream = torch.cuda.Stream(dev)
            pending = {}

            def prefetch(k):
                params = [sample_params(a.src_frames, a.src_h, a.src_w, a.frames, a.crop, True, generator=gen)
                          for _ in range(B)]
                free = torch.cuda.Event()
                free.record()   # everything issued so far (the last reader of this buffer) precedes the refill
                with torch.cuda.stream(pstream):
                    pstream.wait_event(free)
                    xs = preps[k % 2](frames, params)
                    ready = torch.cuda.Event()
                    ready.record(pstream)
                pending[k] = (xs, ready)

            def batch(k):
                if k not in pending:
                    prefetch(k)
                xs, ready = pending.pop(k)
                torch.cuda.current_stream().wait_event(ready)
                prefetch(k + 1)
                return xs

        def labels_of(k):
            return host_labels[0] if a.source == "host" else labels_all[k % 64]

        if a.graph and st.world_size == 1:
            from pytorchvideo_accelerate_amd.engine.graph import GraphedStep

        def step(i, tune=False):
            nonlocal gstep
            xs = batch(-1 if tune else i * a.grad_accum)
            if a.graph and st.world_size == 1 and not tune and i >= 1:
                # captured after the eager tuning step and the first (state-binding) optimizer step; the two
                # preprocessing buffers give two graph keys, captured during warmup
                if gstep is None:
                    gstep = GraphedStep(eng, opt)
                for j in range(a.grad_accum):
                    if j:
                        xs = batch(i * a.grad_accum + j)
                    last = j == a.grad_accum - 1
                    loss, kept["logits"] = gstep(xs, labels_all[(i * a.grad_accum + j) % 64],
                                                 loss_scale=1.0 / a.grad_accum, accumulate=j > 0, optimizer_step=last)
                return loss
            if tune:
                # untimed autotuning pass: every conv geometry is tuned (ranks agree on the choice) with
                # no gradient all-reduce in flight and no optimizer step (weights stay rank-identical)
                sync.begin(False)
                eng.forward_backward(xs, labels_of(0), accumulate=False)
                return None
            opt.zero_grad()
            ls = scaler.get_scale() if scaler is not None else 1.0
            for j in range(a.grad_accum):
                if j:
                    xs = batch(i * a.grad_accum + j)
                last = j == a.grad_accum - 1
                sync.begin(last)
                loss, kept["logits"] = eng.forward_backward(xs, labels_of(i * a.grad_accum + j),
                                                            loss_scale=ls / a.grad_accum)
                sync.finish()
            if i == 0 and a.dump:
                dump["grad"] = eng.flat.grad.clone()
            with trace_range("sgd"):
                if scaler is not None:   # unscale + non-finite check inside the fused SGD; skipped steps back off
                    scaler.step(opt)
                    scaler.update()
                    skipped[0] += int(opt.step_was_skipped)
                else:
                    opt.step()
            return loss

    if not a.plumbing:
        step(0, tune=True)
    for i in range(max(a.warmup, 1)):
        step(i)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    st.barrier()
    if dev.type == "cuda":
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
    sync.stats(reset=True)
    times = []
    t0 = time.perf_counter()
    for i in range(a.steps):
        if dev.type == "cuda":
            ev0 = torch.cuda.Event(enable_timing=True)
            ev1 = torch.cuda.Event(enable_timing=True)
            ev0.record()
            with trace_range(f"step{i}"):
                loss = step(a.warmup + i)
            ev1.record()
            times.append((ev0, ev1))
        else:
            s0 = time.perf_counter()
            loss = step(a.warmup + i)
            times.append((time.perf_counter() - s0) * 1e3)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    st.barrier()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    step_ms = sorted(e0.elapsed_time(e1) for e0, e1 in times) if dev.type == "cuda" else sorted(times)
    p50 = step_ms[len(step_ms) // 2] if step_ms else 0.0
    comm = sync.stats()
    el = torch.tensor([elapsed], device=dev if st.backend == "nccl" else "cpu")
    st.all_reduce_(el, "max")
    elapsed = float(el.item())
    ms_per_step = elapsed * 1000.0 / max(a.steps, 1)
    clips = B * a.grad_accum * st.world_size * a.steps / elapsed if a.steps else 0.0
    if a.dump:
        dump["params"] = opt.flat.data.clone()
        gathered = [torch.zeros_like(dump["params"]) for _ in range(st.world_size)]
        if st.multi:
            import torch.distributed as dist
            dist.all_gather(gathered, dump["params"])
        else:
            gathered = [dump["params"]]
        if st.is_main_process:
            torch.save({"grad": dump["grad"].cpu(), "params": [g.cpu() for g in gathered],
                        "world_size": st.world_size}, a.dump)
    if a.dump_outputs and st.is_main_process and a.steps:
        dump_outputs(a.dump_outputs, {"loss": loss, "logits": kept.get("logits"), "params": opt.flat.data})
    if st.is_main_process:
        headline = ((a.model, a.depth, a.frames, a.crop, a.alpha) == ("slowfast", 50, 32, 224, 4)
                    and not a.plumbing)
        mname = (f"Slow-R50 {a.frames}x{64 // a.frames}x{a.crop}" if a.model == "slow_r50" else
                 f"SlowFast-R{a.depth} {a.frames}x2x{a.crop}")
        fp16 = {"loss_scale": scaler.get_scale(), "skipped_steps": skipped[0]} if scaler is not None else {}
        print(json.dumps({
            "metric": METRIC if headline else f"clips/sec (whole node) {mname}; step-time p50",
            "value": round(clips, 2),
            "unit": "clips/s",
            "n_gpus": st.world_size,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "step_time_p50_ms": round(p50, 3),
            "higher_is_better": True,
            "scaling": "weak",
            # the stock baseline is measured on the headline config only
            "vs_baseline": (round(clips / (STOCK_CLIPS_PER_S_1GPU * st.world_size), 3)
                            if headline and a.precision == "bf16" else None),
            "dtype": "fp32" if a.plumbing else a.precision,
            "data": ("synthetic normal clips, CPU plumbing run" if a.plumbing else
                     "synthetic normalised fp32 clips resident on the device (two batches alternated; NCTHW->NDHWC "
                     "layout pass inside the step); random-init weights" if a.precision == "fp32" else
                     "synthetic uint8 raw-frame .npy corpus (64x256x340 per video) read by the native C++ reader into "
                     "pinned memory, H2D on a copy stream, on-device preprocessing; random-init weights"
                     if a.source == "host" else
                     "synthetic uint8 decoded clips (64x256x340), on-device preprocessing (next batch prefetched "
                     "on a side stream); random-init weights"),
            "config": {"model": mname,
                       "global_batch": B * a.grad_accum * st.world_size,
                       "per_gpu_batch": B, "grad_accum": a.grad_accum, "seq_len": a.frames,
                       "parallelism": f"dp{st.world_size}", "backend": st.backend or "none",
                       "comm": "framework-rccl" if st.comm is not None else ("process-group" if st.multi else "none"),
                       "forced_sync": st.forced,
                       "grad_dtype": a.grad_dtype, "classes": a.classes, "hip_graph": bool(gstep is not None),
                       "deterministic": a.deterministic, "source": a.source,
                       "final_loss": round(float(loss), 4) if loss is not None else None,
                       "peak_mem_gb": (round(torch.cuda.max_memory_allocated(dev) / 2**30, 1)
                                       if dev.type == "cuda" else None),
                       **fp16, **comm},
        }), flush=True)
    st.destroy()


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    a = parse(argv)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(a, argv))
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    if ws != a.gpus:
        print(f"bench.py: WORLD_SIZE={ws} but --gpus {a.gpus}", file=sys.stderr)
    run(a)


if __name__ == "__main__":
    main()
