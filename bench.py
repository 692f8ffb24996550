#!/usr/bin/env python3
"""bench.py — separated utterances/s of the reverse-diffusion hot path on N MI355X of one node.

A "step" = one full pass of the hot path over one resident batch per GPU:
    normalize_batch -> PC sampler (N=30 reverse steps, 1 ald2 corrector step => 60 network
    evaluations, on-device Philox noise) -> scale_output [-> RCCL gather of the waveforms to rank 0]
on B=16 synthetic 4 s / 8 kHz 2-speaker mixtures per GPU (BASELINE.json configs[1]), NCSN++ nf=64
with random-init weights (no checkpoint can be downloaded here), 16-bit activations / weights with fp32
accumulation (--dtype f16, the default: IEEE half precision; bf16: the same kernels on bfloat16 tensors).  Utterances shard embarrassingly: every rank owns its own 16 utterances (weak
scaling) and the only collective is the result gather.

    python bench.py [--gpus N --steps K --warmup W] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

--scaling strong: a FIXED set of --utterances synthetic mixtures of different lengths (3 .. 6 s) is split over the
ranks (length-balanced deal, evaluate_mp.py:495-518 semantics with the imbalance included), every rank separates its
share in width-bucketed batches, and ONE gather at the end collects the per-utterance results; a step = one pass over
the whole set; the line carries per-rank busy times and their imbalance.

A plain run sets up, warms up, times the K steps and prints ONE JSON line (rank 0): `value` (utterances/s), `ms_per_step`
(wall time of one timed step) and the configuration.  --dump-outputs DIR also writes the separated waveforms of the last timed
step (what a caller of the step receives; on several ranks the gathered ones of rank 0) as DIR/separated.npy, float32; the
inputs (synthetic mixtures, weights, per-step noise seeds) depend only on the arguments, so two builds compare output for output.

--full adds everything else the line has carried (each object can be dropped again with its --no-* option):
  one_batch_alone_ms / in_flight_bit_identical — latency of one batch alone, and the same batch again with the other
                 batches in flight (must be bit-identical).
  roofline     — the MFMA kernel instantiation with the most GPU time, named by its real template arguments (round 3:
                 the register-weight 3x3 convolution conv3x3_rw_kernel<2,4,0,2,2>, 128 -> 64 couts with GroupNorm + SiLU):
                 algorithmic FLOPs of its launches / their summed durations, measured with HIP events on the launch
                 stream in one extra, untimed pass of the same step right after the timed region
                 (diffsep_engine_profile_begin / _end / _records); per_shape = the same for every (instantiation, shape)
                 at >= 128 x 128; traffic / pmc = HBM bytes and MFMA utilisation per shader cycle of that instantiation
                 from the committed rocprofv3 --pmc passes (profiles/pmc_conv3x3.json, profiles/r03_pmc_mfma_util.json).
  cpu_baseline — the CPU oracle (torch fp32, this repo's restatement of the reference path) timed on
                 the host cores for a bounded number of network evaluations and scaled to utt/s.
  precision / <other>_mode / fp32_parity_mode / split_parity_mode — the same step in the other precision modes on the
                 driver's clock, and every mode's agreement with the exact fp32 engine's output on the same noise (SI-SDR,
                 relative and absolute RMS).  The parity bar is 1e-3 absolute RMS on the waveforms; on the quiet synthetic
                 outputs (RMS 0.014) that alone would pass a 2.6 % relative error, so value_parity_grade = the fastest
                 mode inside 1e-3 absolute AND 1 % relative RMS (>= 40 dB) of the fp32 engine.
  nf128        — the published model width (nf = 128) in the main dtype: utt/s, one batch alone, dominant kernel.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "diffusion-separation_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GFLOP_PER_NFE = {64: 133.83, 128: 532.89}  # SURVEY.md §8d, per utterance at W=256 (probe-counted 2*MAC)
PEAK_TFLOPS = {"bf16": 2500.0, "f16": 2500.0, "f32": 157.3, "split": 2500.0 / 3}  # MI355X_MICROARCH.md: dense MFMA peaks (split: 3 bf16 MFMAs per product)
HBM_PEAK_BPS = 8.0e12                          # MI355X_MICROARCH.md: HBM3E ~8 TB/s
DUMP_MAX_BYTES = 64_000_000                    # --dump-outputs: at most this much per run


def dump_outputs(path, name, t):
    """Write tensor t as path/name.npy (float32).  A tensor larger than DUMP_MAX_BYTES is written as a fixed sample of its
    flattened values (every k-th element, k the smallest stride that fits), the same elements for the same arguments."""
    a = t.detach().float().cpu().numpy()
    if a.nbytes > DUMP_MAX_BYTES:
        a = a.reshape(-1)[::-(-a.size // (DUMP_MAX_BYTES // 4))]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))

def cpu_baseline(nf, T, N, corrector_steps):
    """The CPU oracle (this repo's torch-fp32 restatement of the reference path, validated against the imported reference in the
    build container) separating ONE utterance end to end on the host cores: normalize_batch -> the full PC sampler (N reverse
    steps x (corrector + predictor) = N (corrector_steps + 1) network evaluations on injected noise) -> scale_output, exactly the
    work of one row of a GPU step.  Returns (seconds for the utterance, network evaluations, seconds of one evaluation, threads)."""
    import diffsep_oracle as O
    from diffsep_amd import synth
    torch.set_grad_enabled(False)
    cfg = O.default_config(nf, 2)
    p = O.to_torch(synth.synth_state_dict(O.param_table(cfg), 7))
    mix = torch.from_numpy(synth.synth_batch(1, T=T)[0])
    mix_norm, _, _ = O.normalize_batch(mix)
    xt = O.prior_sampling(cfg, mix_norm, torch.from_numpy(synth.synth_noise("cpu.z", (1, 2, T))))
    t = torch.tensor([0.5])
    O.score_forward(p, cfg, xt, t, mix_norm)  # warm-up (oneDNN primitive creation)
    # torch's default (= all hardware threads) is not the fastest setting on many-core hosts for these
    # small convolutions: try a few thread counts briefly and keep the best one for the timed run.
    ncpu = torch.get_num_threads()
    best, best_t = ncpu, None
    for nt in sorted({ncpu, max(1, ncpu // 2), max(1, ncpu // 4), min(ncpu, 32), min(ncpu, 16)}, reverse=True):
        torch.set_num_threads(nt)
        O.score_forward(p, cfg, xt, t, mix_norm)
        t1 = time.perf_counter()
        O.score_forward(p, cfg, xt, t, mix_norm)
        d = time.perf_counter() - t1
        if best_t is None or d < best_t:
            best, best_t = nt, d
    torch.set_num_threads(best)
    draws = [torch.from_numpy(synth.synth_noise(f"cpu.z{i}", (1, 2, T))) for i in range(1 + N * (corrector_steps + 1))]
    t0 = time.perf_counter()
    out, nfe = O.separate(p, cfg, mix, draws, N=N, corrector_steps=corrector_steps, snr=0.5, eps=0.03, denoise=True)
    dt = time.perf_counter() - t0
    assert bool(torch.isfinite(out).all())
    return dt, int(nfe), best_t, best


def run_strong(args, engs, ops, on_stream, sync, fence, dist, world, rank, dev, sde, dry):
    """--scaling strong: a fixed set of utterances of different lengths split over the ranks; a step = one pass over
    the whole set; one gather of the separated waveforms at the end of a step."""
    from diffsep_amd import synth
    from diffsep_amd.dist_utils import rank_indices
    from diffsep_amd.evaluate import plan_batches
    n, S, K = args.utterances, 2, len(engs)
    lengths = [24000 + (i * 7919) % 24001 for i in range(n)]          # 3 .. 6 s at 8 kHz
    mine = rank_indices(n, world, rank, lengths, balance=True)          # sorted by length, dealt round-robin
    e0 = engs[0]
    batches = plan_batches(mine, lengths, e0.padded_frames, args.batch)
    staged = []
    for g in batches:                                                    # resident in HBM before timing
        Tb = e0.bucket_length(e0.padded_frames(max(lengths[i] for i in g)))
        mix = torch.zeros((len(g), 1, Tb))
        for b, i in enumerate(g):
            mix[b, :, :lengths[i]] = torch.from_numpy(synth.synth_mixture(i, T=lengths[i])[0])
        staged.append((g, [lengths[i] for i in g], mix.to(dev)))
    if batches:
        for e in engs:
            e.reserve(max(len(g) for g in batches), max(m.shape[-1] for _, _, m in staged))
    nloc_max = (n + world - 1) // world
    Tmax = e0.bucket_length(e0.padded_frames(max(lengths)))
    block = torch.zeros((nloc_max, S, Tmax), dtype=torch.float32, device=dev)
    blocks = [torch.empty_like(block) for _ in range(world)] if rank == 0 and world > 1 else None
    keep = [None] * K
    nfe = 0

    def one_pass(p):
        nonlocal nfe
        row = 0
        for j, (g, lens, mix) in enumerate(staged):
            w = j % K
            with on_stream(w):
                mixn = torch.zeros_like(mix)
                for b, L in enumerate(lens):
                    mixn[b, :, :L] = ops.normalize_batch(mix[b:b + 1, :, :L])[0][0]
                sep, nfe = engs[w].pc_sample(mixn, sde, N=args.N, corrector_steps=args.corrector_steps, snr=0.5, eps=0.03,
                                             denoise=True, lengths=lens, seeds=[10_000 * (p + 1000) + i for i in g])
                for b, L in enumerate(lens):
                    block[row + b, :, :L] = ops.scale_output(mix[b:b + 1, :, :L], sep[b:b + 1, :, :L])[0]
            keep[w] = (mixn, sep)
            row += len(g)
        sync()

    for p in range(max(1, args.warmup)):   # plans + graph captures for every (B, W) of this rank's share
        one_pass(-1 - p)
    fence()
    busy = 0.0
    t0 = time.perf_counter()
    for p in range(args.steps):
        tb = time.perf_counter()
        one_pass(p)
        busy += time.perf_counter() - tb
        if world > 1:
            dist.gather(block, blocks, dst=0)   # ONE collective per pass (RCCL over xGMI)
    fence()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, "separated", torch.cat(blocks) if blocks else block)
    finite = bool(torch.isfinite(block).all())
    busy_all = [busy]
    if world > 1:
        tt = torch.tensor([elapsed, busy], dtype=torch.float64, device=dev)
        parts = [torch.zeros_like(tt) for _ in range(world)]
        dist.all_gather(parts, tt)
        elapsed = max(float(q[0]) for q in parts)
        busy_all = [float(q[1]) for q in parts]
    ranks_seen = seen_ranks(dist, world, rank, int(os.environ.get("LOCAL_RANK", "0")), dev) if world > 1 else [[0, 0]]
    # which utterance sits in which row of the gathered blocks (untimed bookkeeping: every utterance must arrive exactly once)
    rows = [i for g, _, _ in staged for i in g]
    idx = torch.full((nloc_max,), -1, dtype=torch.int64, device=dev)
    if rows:
        idx[:len(rows)] = torch.tensor(rows, dtype=torch.int64, device=dev)
    idx_all = [idx]
    if world > 1:
        idx_all = [torch.empty_like(idx) for _ in range(world)]
        dist.all_gather(idx_all, idx)
    got = [int(v) for q in idx_all for v in q.tolist() if int(v) >= 0]
    if rank == 0:
        value = n * args.steps / elapsed
        secs = sum(lengths) / 8000.0
        print(json.dumps({
            "metric": "separated utterances/sec (3-6 s, 8 kHz, 2-spk, N=30 PC steps), fixed set split over the GPUs",
            "value": round(value, 4), "unit": "utterances/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 2), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "configs[2]-shaped: %d utterances of 3-6 s @ 8 kHz (mean %.2f s), N=%d + %d ald2 corrector "
                                   "step, NCSN++ nf=%d random-init; length-balanced deal to the ranks, width-bucketed batches "
                                   "of <= %d, %d batches in flight per GPU, one gather per pass"
                                   % (n, secs / n, args.N, args.corrector_steps, args.nf, args.batch, K),
                       "utterances": n, "batch_per_gpu": args.batch, "N": args.N, "corrector_steps": args.corrector_steps,
                       "nf": args.nf, "sharding": "utterances/%d (length-balanced)" % world, "batches_in_flight": K},
            "realtime_factor": round(secs * args.steps / elapsed, 2),
            "rank_busy_s_per_step": [round(b / args.steps, 4) for b in busy_all],
            "imbalance_max_over_mean": round(max(busy_all) / (sum(busy_all) / len(busy_all)), 4),
            "gathered_utterances": len(got), "gathered_unique": len(set(got)),
            "engine_calls_rank0_per_step": len(staged), "nfe_per_call": int(nfe), "finite": finite,
            "ranks_seen": ranks_seen}), flush=True)


def seen_ranks(dist, world, rank, local_rank, dev):
    """[rank, local device index] of every participating rank, collected with one all-gather."""
    me = torch.tensor([rank, local_rank], dtype=torch.int64, device=dev)
    parts = [torch.zeros_like(me) for _ in range(world)]
    dist.all_gather(parts, me)
    return [[int(q[0]), int(q[1])] for q in parts]


def self_launch(n):
    """Re-run this command line as n ranks (evaluate_mp.py:495-518: one worker per GPU)."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("GPU_MAX_HW_QUEUES", "8")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16, help="utterances per GPU")
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16", "f32", "split"],
                    help="f16 (default): 16-bit tensors in IEEE half precision (the half-precision build of the library); bf16: "
                         "the same kernels on bfloat16 tensors; f32 / split: fp32 tensors")
    ap.add_argument("--samples", type=int, default=32000, help="samples per utterance (4 s at 8 kHz)")
    ap.add_argument("-N", type=int, default=30)
    ap.add_argument("--corrector-steps", type=int, default=1)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure and check everything else: one batch alone and bit identity in "
                         "flight, roofline, the other precision modes, nf = 128, the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the separated waveforms of the last timed step as DIR/separated.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline pass")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-extra-modes", action="store_true", help="with --full: skip the other precision modes and the nf = 128 section")
    ap.add_argument("--no-nf128", action="store_true", help="with --full: skip the nf = 128 section")
    ap.add_argument("--no-rw-quarter", action="store_true", help="keep every register-weight launch on all CUs even with several batches in flight")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"])
    ap.add_argument("--utterances", type=int, default=128, help="--scaling strong: size of the fixed utterance set")
    ap.add_argument("--in-flight", type=int, default=4,
                    help="batches in flight per GPU: step i runs on engine / HIP stream i %% K, so consecutive steps overlap "
                         "(the ~110 small launches of one batch's NFE leave the chip mostly idle; another batch's large "
                         "convolutions fill it).  1 = one batch at a time.  Every step is still a full batch through the "
                         "whole path and all timed steps finish inside the timed region.")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    # HIP maps streams onto GPU_MAX_HW_QUEUES (default 4, one taken by the null stream) hardware queues; read when the
    # runtime initialises, i.e. before the first torch.cuda call
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # plain `python bench.py --gpus N`: launch the N ranks ourselves (one process per GPU under
        # torch.distributed.run, rendezvous on 127.0.0.1 and a free port) and pass their output through; rank 0
        # of the children prints the one JSON line
        sys.exit(self_launch(args.gpus))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d does not match WORLD_SIZE=%d" % (args.gpus, world))
    import torch.distributed as dist
    # DIFFSEP_BENCH_DRYRUN=1: the same control flow (collectives, barriers, who prints) on CPU tensors over gloo with a
    # stand-in for the engine — only for the world_size-2 test of the multi-rank sequencing, never a measurement
    dry = os.environ.get("DIFFSEP_BENCH_DRYRUN") == "1"
    dev = "cpu" if dry else "cuda"
    if not dry:
        torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if dry:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    from diffsep_amd import synth
    torch.set_grad_enabled(False)
    B, T, S = args.batch, args.samples, 2
    if dry:
        import contextlib
        import types

        class _Eng:  # records nothing, computes nothing
            def pc_sample(self, mix_norm, sde, N, corrector_steps, **kw):
                return torch.zeros((mix_norm.shape[0], S, mix_norm.shape[-1])), N * (corrector_steps + 1)
            def padded_frames(self, T): return 64 * ((1 + (T + 382) // 128 + 63) // 64)
            def bucket_length(self, W): return 128 * W - 383
            def reserve(self, B, T): pass
            def profile_begin(self): pass
            def profile_end(self): return {"conv3x3_8x32xN64": (1.0, 1.0, 1, 1.0)}
            def profile_records(self): return []
            def device_bytes(self): return 0
        K = max(1, args.in_flight)
        engs = [_Eng() for _ in range(K)]
        per_engine, hbm_free, hbm_total = 0, 0, 0
        ops = types.SimpleNamespace(normalize_batch=lambda m: (m, None, None), scale_output=lambda m, s: s)
        on_stream = lambda w: contextlib.nullcontext()
        sync = lambda: None
        gstream = None
    else:
        from diffsep_amd import _lib, ops
        from diffsep_amd.engine import Engine, pack_state_dict, param_table
        dt_flag = {"bf16": _lib.BF16, "f16": _lib.F16, "f32": _lib.F32, "split": _lib.F32_SPLIT}[args.dtype]
        cfg = _lib.model_config(nf=args.nf, num_sources=S, dtype=dt_flag)
        sd = synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], 7)
        K = max(1, args.in_flight)
        blob = pack_state_dict(cfg, sd)
        # every rank keeps K engines (weights + a ~3.3 GB workspace each at nf = 64, B = 16: 14 GB of the 288 GB at K = 4; eight
        # ranks on eight GPUs hold eight such sets, one per device).  The first engine is measured and K is capped by what
        # the device has free, so that a crowded GPU degrades to fewer batches in flight instead of failing to allocate.
        engs = [Engine(cfg, blob)]  # (engines before streams: hardware queues go in creation order)
        engs[0].reserve(B, T)
        per_engine = engs[0].device_bytes()
        hbm_free, hbm_total = torch.cuda.mem_get_info()
        k_fit = 1 + int(max(0, hbm_free - (2 << 30)) // max(per_engine, 1))
        if k_fit < K:
            print("bench.py: rank %d: %d batches in flight asked, HBM has room for %d engines of %.1f GB" % (rank, K, k_fit, per_engine / 1e9),
                  file=sys.stderr, flush=True)
            K = max(1, k_fit)
        engs += [Engine(cfg, blob) for _ in range(K - 1)]
        # Throughput mode for several engines on one GPU (round 5; what evaluate / separate --streams K > 1 set through
        # DiffSepModel.set_throughput_mode; same arithmetic, other grouping of the GroupNorm partial sums: tests/test_round6_gpu.py): a register-weight convolution whose blocks would get <= 4 tiles
        # (the 128-row level at B = 16: a 295 KB weight prologue per 4 tiles) runs on a QUARTER of the CUs with four times the tiles
        # per block; the other batches' kernels take the rest of the chip.  Same box, interleaved: 80.9 -> 82.9 utt/s with four batches
        # in flight, 260 -> 300 ms for one batch alone — so it is an option of the multi-stream callers, not a default of the engine.
        spread = K > 1 and not args.no_rw_quarter
        if spread:
            for e in engs:
                e.set_option("rw_quarter", 1)
        if args.no_graph:
            for e in engs:
                e.set_graph(False)
        streams = [torch.cuda.Stream() for _ in range(K)]
        on_stream = lambda w: torch.cuda.stream(streams[w])
        sync = torch.cuda.synchronize
        # the result gather runs on ONE dedicated stream per rank (after an event of the producing stream): every
        # rank issues its collectives in step order on a single stream, whatever the number of batches in flight
        gstream = torch.cuda.Stream() if world > 1 else None
    sde = dict(ndim=S, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5)

    def fence():
        sync()
        if world > 1:
            dist.barrier()
        sync()

    if args.scaling == "strong":
        run_strong(args, engs, ops, on_stream, sync, fence, dist, world, rank, dev, sde, dry)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return
    mix = torch.from_numpy(synth.synth_batch(B, T=T, start=rank * B)[0]).to(dev)  # resident before timing
    eng = engs[0]
    # one set of gather buffers per batch in flight (rank 0)
    gathered = [[torch.empty((B, S, T), dtype=torch.float32, device=dev) for _ in range(world)] if rank == 0 else None
                for _ in range(K)]
    keep = [None] * K  # the tensors of a worker's last step stay referenced until its stream has drained

    def step(i, collect=True, w=None, seed=None):
        w = i % K if w is None else w
        with on_stream(w):
            mix_norm, _, _ = ops.normalize_batch(mix)
            sep, nfe = engs[w].pc_sample(mix_norm, sde, N=args.N, corrector_steps=args.corrector_steps, snr=0.5,
                                         eps=0.03, denoise=True, seed=1000 + i if seed is None else seed)
            out = ops.scale_output(mix, sep)
            if world > 1 and collect:
                if gstream is None:
                    dist.gather(out, gathered[w], dst=0)
                else:
                    ev = torch.cuda.Event()
                    ev.record()
                    gstream.wait_event(ev)
                    with torch.cuda.stream(gstream):
                        dist.gather(out, gathered[w], dst=0)  # RCCL over xGMI: the only collective on the path
                    # `out` was allocated on worker stream w and is read by the collective on gstream: tell the caching
                    # allocator, so the block is not handed back to stream w before the gather has finished with it
                    out.record_stream(gstream)
                    if gathered[w] is not None:
                        for g_ in gathered[w]:
                            g_.record_stream(gstream)
        keep[w] = (mix_norm, sep, out)
        return out, nfe

    # engine preparation (not a step of the benchmark): workspace plan, then hipGraph capture, for every engine
    for w in range(K):
        for _ in range(2):
            step(w, collect=False)
    fence()
    for i in range(args.warmup):
        out, nfe = step(i)
    fence()
    t0 = time.perf_counter()
    outs = []
    for i in range(args.steps):
        out, nfe = step(args.warmup + i)
        outs.append(out)
    fence()
    elapsed = time.perf_counter() - t0
    finite = all(bool(torch.isfinite(o).all()) for o in outs[-K:])
    if args.dump_outputs and rank == 0:
        last = gathered[(args.warmup + args.steps - 1) % K]
        dump_outputs(args.dump_outputs, "separated", torch.cat(last) if world > 1 else outs[-1])
    del outs
    alone_spread_ms = alone_ms = same_bits = None
    if args.full:
        # latency of ONE batch with nothing else in flight (untimed extra): in the throughput mode of the timed region, then —
        # what one_batch_alone_ms and the per-kernel roofline below report — in the engine's default configuration (every
        # launch on all CUs)
        if not dry and spread:
            fence()
            t1 = time.perf_counter()
            step(0, collect=False, w=0, seed=77)
            sync()
            alone_spread_ms = (time.perf_counter() - t1) * 1e3
            engs[0].set_option("rw_quarter", 0)
            for _ in range(2):   # plan + graph capture of the default configuration
                step(0, collect=False, w=0, seed=77)
            sync()
        fence()
        t1 = time.perf_counter()
        ref_out, _ = step(0, collect=False, w=0, seed=77)
        sync()
        alone_ms = (time.perf_counter() - t1) * 1e3
        # the same batch and seed again with K-1 other batches in flight: must be bit-identical (untimed check)
        again = [step(j, collect=False, w=j, seed=77 + j)[0] for j in range(K)]
        sync()
        same_bits = bool(torch.equal(again[0], ref_out))
        del again, ref_out

    roof = None
    if args.full and not args.no_roofline and rank == 0:
        eng.profile_begin()
        step(10_000, collect=False, w=0)  # rank 0 only: no collective in this untimed pass
        prof = eng.profile_end()
        recs = eng.profile_records()
        dom = max(prof, key=lambda k: prof[k][1])  # the kernel class with the most GPU time
        fl, ms, n, by = prof[dom]
        tot_ms = sum(v[1] for v in prof.values())
        ach = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        peak = PEAK_TFLOPS[args.dtype]
        traffic, traffic_source = None, None
        # the bound is whichever floor of an average launch is higher: HBM at 8 TB/s or dense MFMA at `peak`
        hbm_floor_us = by / max(n, 1) / HBM_PEAK_BPS * 1e6
        mfma_floor_us = fl / max(n, 1) / (peak * 1e12) * 1e6
        # per (kernel instantiation, problem shape): launches, average duration, fractions of both roofs; the
        # instantiation (real template arguments) with the most GPU time names the roofline object
        by_shape, by_kernel = {}, {}
        for r in recs:
            if r["cls"] < 0:
                continue
            key = (r["kernel"], r["taps"], r["Cin"], r["Cout"], r["H"], r["W"], r["skip_cin"], r["has_res"])
            a = by_shape.setdefault(key, [0, 0.0, 0.0, 0.0])
            a[0] += 1; a[1] += r["ms"]; a[2] += r["flops"]; a[3] += r["bytes"]
        per_shape = []
        for (kn, taps, ci, co, H_, W_, sk, hr), (n_, ms_, fl_, by_) in sorted(by_shape.items(), key=lambda kv: -kv[1][1]):
            if ms_ <= 0 or H_ * W_ < 128 * 128:
                continue
            per_shape.append({"kernel": kn, "shape": "%dx%d %d->%d%s%s @%dx%d" % (3 if taps == 9 else 1, 3 if taps == 9 else 1, ci, co,
                                                                                  " +skip%d" % sk if sk else "", " +res" if hr else "", H_, W_),
                              "launches": n_, "avg_us": round(ms_ / n_ * 1e3, 1),
                              "frac_mfma": round(fl_ / (ms_ * 1e-3) / 1e12 / peak, 4),
                              "frac_hbm": round(by_ / (ms_ * 1e-3) / HBM_PEAK_BPS, 4),
                              # the roof that bounds THIS shape = the higher of its two floors (64-cout layers at 256^2
                              # sit at the machine balance: their HBM floor is the higher one)
                              "bound": "hbm" if by_ / HBM_PEAK_BPS > fl_ / (peak * 1e12) else "mfma"})
        # SURVEY 8(d), second half: the HBM-bound launches of the step against the HBM roof, one entry per (kernel, shape):
        # algorithmic bytes (inputs read once, outputs written once) over the summed HIP-event durations of the same pass
        hbm_shape = {}
        for r in recs:
            if r["cls"] >= 0:
                continue
            a = hbm_shape.setdefault((r["kernel"], r["Cin"], r["H"], r["W"]), [0, 0.0, 0.0])
            a[0] += 1; a[1] += r["ms"]; a[2] += r["bytes"]
        hbm_kernels = [{"kernel": kn, "shape": "C=%d @%dx%d" % (c_, H_, W_), "launches": n_, "avg_us": round(ms_ / n_ * 1e3, 2),
                        "algorithmic_bytes_per_launch": by_ / n_, "gb_per_s": round(by_ / (ms_ * 1e-3) / 1e9, 1),
                        "frac_hbm": round(by_ / (ms_ * 1e-3) / HBM_PEAK_BPS, 4), "total_ms": round(ms_, 3)}
                       for (kn, c_, H_, W_), (n_, ms_, by_) in sorted(hbm_shape.items(), key=lambda kv: -kv[1][1]) if ms_ > 0]
        recs = [r for r in recs if r["cls"] >= 0]
        by_shape, by_kernel = {}, {}
        for r in recs:
            key = (r["kernel"], r["taps"], r["Cin"], r["Cout"], r["H"], r["W"], r["skip_cin"], r["has_res"])
            a = by_shape.setdefault(key, [0, 0.0, 0.0, 0.0])
            a[0] += 1; a[1] += r["ms"]; a[2] += r["flops"]; a[3] += r["bytes"]
            b_ = by_kernel.setdefault(r["kernel"], [0, 0.0, 0.0, 0.0])
            b_[0] += 1; b_[1] += r["ms"]; b_[2] += r["flops"]; b_[3] += r["bytes"]
        dom_k = max(by_kernel, key=lambda k: by_kernel[k][1]) if by_kernel else None
        kname = dom_k or dom
        if dom_k:  # the roofline object describes this one instantiation
            n, ms, fl, by = by_kernel[dom_k]
            ach = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            hbm_floor_us = by / max(n, 1) / HBM_PEAK_BPS * 1e6
            mfma_floor_us = fl / max(n, 1) / (peak * 1e12) * 1e6
        # HBM bytes per launch of that instantiation from the committed PMC passes (FETCH_SIZE / WRITE_SIZE, separate runs of
        # tools/pmc_traffic.sh with the guide's correction 2 * FETCH + WRITE), and its MFMA utilisation per shader cycle
        pmc_util = None
        try:
            pj = json.load(open(os.path.join(ROOT, "profiles", "pmc_conv3x3.json")))
            ent = pj.get("by_instantiation", {}).get(kname) if pj.get("dtype") == args.dtype and args.nf == 64 and B == 16 else None
            if ent:
                traffic = ent["hbm_bytes_per_launch_guide_formula"]
                traffic_source = ("profiles/pmc_conv3x3.json = output of `COMMIT=%s bash tools/pmc_traffic.sh` (rocprofv3 --kernel-trace --pmc "
                                  "FETCH_SIZE / --pmc WRITE_SIZE in separate passes around `python bench.py --steps 1 --warmup 0 -N 4 --in-flight 1 "
                                  "--no-graph`, guide correction 2*FETCH + WRITE, average over the %d launches of this instantiation; the "
                                  "profiler cannot wrap the N = 30 run of this line: rocprofv3 --pmc crashes on it, so the counters come from "
                                  "that separate, committed run of the same kernels and launch mix)" % (pj.get("commit"), ent["launches"]))
        except Exception:
            traffic = traffic_source = None
        try:
            pmc_file = next(f_ for f_ in ("r06_pmc_mfma_util.json", "r05_pmc_mfma_util.json", "r04_pmc_mfma_util.json")
                            if os.path.exists(os.path.join(ROOT, "profiles", f_)))
            pu = json.load(open(os.path.join(ROOT, "profiles", pmc_file)))
            for k_, v_ in pu.get("kernels", {}).items():
                if k_.split(" grid ")[0] == kname and pu.get("dtype") == args.dtype:
                    pmc_util = {"mfma_util_per_shader_cycle": v_.get("mfma_util"), "shader_clock_ghz": v_.get("shader_clock_ghz"),
                                "mfma_busy_per_wave_cycle": v_.get("mfma_busy_per_wave_cycle"),
                                "valu_per_mfma": v_.get("valu_per_mfma"), "lds_per_mfma": v_.get("lds_per_mfma"),
                                "lds_bank_conflict_cycles_per_lds_inst": v_.get("lds_bank_conflict_cycles_per_lds_inst"),
                                "source": "profiles/%s = output of `COMMIT=%s bash tools/pmc_util.sh` (two rocprofv3 "
                                          "--kernel-trace --pmc passes around the N = 4, one-in-flight, eager variant of this command; a "
                                          "separate, committed run)" % (pmc_file, pu.get("commit"))}
        except Exception:
            pmc_util = None
        if hbm_floor_us > mfma_floor_us:
            gbs = by / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
            roof = {"bound": "hbm", "kernel": kname, "achieved": round(gbs, 1), "peak": HBM_PEAK_BPS / 1e9,
                    "unit": "GB/s", "frac": round(gbs / (HBM_PEAK_BPS / 1e9), 4)}
        else:
            roof = {"bound": "mfma", "kernel": kname, "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s",
                    "frac": round(ach / peak, 4)}
        # the same kernel's average duration in the committed rocprofv3 --kernel-trace --stats summary (profiles/rNN_*_kernel_stats.md):
        # `frac` above comes from the HIP-event pass of THIS run (one batch alone, eager launches); the profile is a separate run of
        # the bench command under the tracer — the two must tell the same story
        roof["frac_rocprof"] = roof["frac_rocprof_source"] = None
        try:
            import re as _re
            for cand in ("r06_bench_%s_alone_kernel_stats.md" % args.dtype, "r06_bench_%s_kernel_stats.md" % args.dtype,
                         "r05_bench_%s_kernel_stats.md" % args.dtype):
                pth = os.path.join(ROOT, "profiles", cand)
                if not os.path.exists(pth) or args.nf != 64 or B != 16:
                    continue
                for line in open(pth):
                    m_ = _re.match(r"\| `(.+?)` \| (\d+) \| ([\d.]+) \| ([\d.]+) \|", line)
                    if m_ and m_.group(1).replace(" ", "") == kname.replace(" ", ""):
                        avg_us = float(m_.group(4))
                        fr = (by / max(n, 1) / (avg_us * 1e-6) / HBM_PEAK_BPS) if roof["bound"] == "hbm" else \
                             (fl / max(n, 1) / (avg_us * 1e-6) / 1e12 / peak)
                        roof["frac_rocprof"] = round(fr, 4)
                        roof["frac_rocprof_source"] = "profiles/%s: %s calls, avg %.2f us" % (cand, m_.group(2), avg_us)
                        break
                if roof["frac_rocprof"] is not None:
                    break
        except Exception:
            pass
        roof.update({"traffic": traffic, "traffic_source": traffic_source, "pmc": pmc_util, "launches": n, "avg_launch_us": round(ms / max(n, 1) * 1e3, 2),
                "flops_per_launch": fl / max(n, 1), "algorithmic_bytes_per_launch": by / max(n, 1),
                "hbm_floor_us": round(hbm_floor_us, 2), "mfma_floor_us": round(mfma_floor_us, 2),
                "achieved_tflops": round(ach, 2),
                "gpu_time_share_of_mfma_kernels": round(ms / tot_ms, 4) if tot_ms > 0 else None,
                "per_shape": per_shape[:24],
                "hbm_kernels": hbm_kernels[:24],
                "hbm_kernels_total_ms": round(sum(h_["total_ms"] for h_ in hbm_kernels), 2),
                "per_instantiation_ms": {k: round(v[1], 2) for k, v in sorted(by_kernel.items(), key=lambda kv: -kv[1][1])[:16]},
                "per_kernel_ms": {k: round(v[1], 2) for k, v in prof.items() if v[2]},
                # every MFMA kernel class of the step against both roofs (algorithmic flops / bytes over its summed time)
                "per_kernel_roofline": {k: {"launches": v[2], "tflops": round(v[0] / (v[1] * 1e-3) / 1e12, 1),
                                            "gb_per_s": round(v[3] / (v[1] * 1e-3) / 1e9, 1),
                                            "frac_mfma": round(v[0] / (v[1] * 1e-3) / 1e12 / peak, 4),
                                            "frac_hbm": round(v[3] / (v[1] * 1e-3) / HBM_PEAK_BPS, 4)}
                                        for k, v in prof.items() if v[2] and v[1] > 0},
                "all_mfma_kernels_ms": round(tot_ms, 2),
                "all_mfma_kernels_tflops": round(sum(v[0] for v in prof.values()) / (tot_ms * 1e-3) / 1e12, 2)})

    extra_json = {}
    if args.full and world == 1 and not dry and not args.no_extra_modes and args.dtype in ("bf16", "f16"):
        # ---- the other precision modes of the same step on the driver's clock (after the main timed region): the other
        # 16-bit storage format, exact fp32, split fp32; and their agreement with the exact fp32 engine on the same seeds
        other = "bf16" if args.dtype == "f16" else "f16"
        K2 = min(K, 2)

        def make(dt_code, n):
            es = [Engine(_lib.model_config(nf=args.nf, num_sources=S, dtype=dt_code), blob) for _ in range(n)]
            if spread and n > 1:  # (the same throughput mode as the main engines; it only touches the 16-bit register-weight launches)
                for e_ in es:
                    e_.set_option("rw_quarter", 1)
            return es

        def run_on(es, i, w):
            with on_stream(w):
                mn, _, _ = ops.normalize_batch(mix)
                sep, _ = es[w].pc_sample(mn, sde, N=args.N, corrector_steps=args.corrector_steps, snr=0.5, eps=0.03,
                                         denoise=True, seed=2000 + i)
                out = ops.scale_output(mix, sep)
            keep[w] = (mn, sep, out)
            return out

        def time_mode(es, nstep):
            for w in range(len(es)):           # plans + graph capture
                run_on(es, w, w)
                run_on(es, w, w)
            sync()
            t2 = time.perf_counter()
            for i in range(nstep):
                run_on(es, i, i % len(es))
            sync()
            return B * nstep / (time.perf_counter() - t2)

        def dominant(es):
            es[0].profile_begin()
            run_on(es, 10_000, 0)
            es[0].profile_end()
            by_k = {}
            for r in es[0].profile_records():
                if r["cls"] < 0:
                    continue
                a_ = by_k.setdefault(r["kernel"], [0, 0.0, 0.0])
                a_[0] += 1; a_[1] += r["ms"]; a_[2] += r["flops"]
            k_ = max(by_k, key=lambda k: by_k[k][1])
            return k_, by_k[k_]

        def si_sdr_db(est, ref):
            est, ref = est.double(), ref.double()
            a = (est * ref).sum(-1, keepdim=True) / (ref * ref).sum(-1, keepdim=True)
            return 10 * torch.log10(((a * ref) ** 2).sum(-1) / ((est - a * ref) ** 2).sum(-1))

        e32, esp = make(_lib.F32, K2), make(_lib.F32_SPLIT, K2)
        eot = make({"bf16": _lib.BF16, "f16": _lib.F16}[other], K)
        ups = {"f32": time_mode(e32, 4), "split": time_mode(esp, 6), other: time_mode(eot, args.steps)}
        mix_norm0 = ops.normalize_batch(mix)[0]
        kw = dict(N=args.N, corrector_steps=args.corrector_steps, snr=0.5, eps=0.03, denoise=True, seed=4242)
        # (compared at the scale of the input waveforms — peak 0.9 — after scale_output, like the parity tests)
        sep_of = lambda e_: ops.scale_output(mix, e_.pc_sample(mix_norm0, sde, **kw)[0])
        o32 = sep_of(e32[0])
        outs_ = {"split": sep_of(esp[0]), other: sep_of(eot[0]), args.dtype: sep_of(engs[0])}
        q = {k: si_sdr_db(v, o32) for k, v in outs_.items()}
        rel = {k: float(((v - o32).double().pow(2).mean() / o32.double().pow(2).mean()).sqrt()) for k, v in outs_.items()}
        absr = {k: float((v - o32).double().pow(2).mean().sqrt()) for k, v in outs_.items()}
        k32, (n32, ms32, fl32) = dominant(e32)
        ksp, (nsp, mssp, flsp) = dominant(esp)
        # hybrid (pl_model dtype="hybrid"): a split engine of the SAME library build evaluates the first HYBRID_HEAD_STEPS
        # reverse steps, the main 16-bit engine the rest
        hyb = None
        if args.dtype == "f16":
            from diffsep_amd.pl_model import HYBRID_HEAD_STEPS
            ehd = [Engine(_lib.model_config(nf=args.nf, num_sources=S, dtype=_lib.F32_SPLIT), blob, lib_kind="f16") for _ in range(K)]

            def run_h(i, w):
                with on_stream(w):
                    mn, _, _ = ops.normalize_batch(mix)
                    sep, _ = engs[w].pc_sample(mn, sde, N=args.N, corrector_steps=args.corrector_steps, snr=0.5, eps=0.03,
                                               denoise=True, seed=2000 + i, tail=ehd[w], head_steps=HYBRID_HEAD_STEPS)
                    out = ops.scale_output(mix, sep)
                keep[w] = (mn, sep, out)
            for w in range(K):
                run_h(w, w); run_h(w, w)
            sync()
            t4 = time.perf_counter()
            for i in range(args.steps):
                run_h(i, i % K)
            sync()
            ups["hybrid"] = B * args.steps / (time.perf_counter() - t4)
            oh = ops.scale_output(mix, engs[0].pc_sample(mix_norm0, sde, tail=ehd[0], head_steps=HYBRID_HEAD_STEPS, **kw)[0])
            q["hybrid"] = si_sdr_db(oh, o32)
            rel["hybrid"] = float(((oh - o32).double().pow(2).mean() / o32.double().pow(2).mean()).sqrt())
            absr["hybrid"] = float((oh - o32).double().pow(2).mean().sqrt())
            hyb = True
            for e_ in ehd:
                e_.close()

        def quality(k):
            return {"si_sdr_db_vs_fp32": round(float(q[k].mean()), 2), "si_sdr_db_vs_fp32_min": round(float(q[k].min()), 2),
                    "rel_rms_vs_fp32": float("%.3e" % rel[k]), "abs_rms_vs_fp32": float("%.3e" % absr[k])}
        extra_json = {
            "precision": {"note": "separated waveforms (input scale: mixture peak 0.9, output RMS %.3f) of each mode against the "
                                  "exact fp32 engine's on the same noise (B = %d, %d NFE); parity-grade = inside 1e-3 absolute "
                                  "AND 1e-2 relative RMS (the fp32 engine itself is 6e-8 from the CPU oracle, tests/test_engine_gpu.py)"
                                  % (float(o32.double().pow(2).mean().sqrt()), B, nfe),
                          args.dtype: quality(args.dtype), other: quality(other), "split": quality("split"),
                          **({"hybrid": quality("hybrid")} if hyb else {})},
            **({"hybrid_mode": {"utt_per_s": round(ups["hybrid"], 3), "batches_in_flight": K, "head_steps": HYBRID_HEAD_STEPS,
                                "note": "split engine for the first head_steps reverse steps, f16 engine after (pl_model dtype='hybrid')"}}
               if hyb else {}),
            other + "_mode": {"utt_per_s": round(ups[other], 3), "batches_in_flight": K,
                              "note": "the same kernels on the other 16-bit storage format (bf16: libdiffsep_hip.so, f16: "
                                      "libdiffsep_hip_f16.so)"},
            "fp32_parity_mode": {"utt_per_s": round(ups["f32"], 3), "batches_in_flight": K2, "kernel": k32,
                                 "frac": round(fl32 / (ms32 * 1e-3) / 1e12 / PEAK_TFLOPS["f32"], 4) if ms32 > 0 else None,
                                 "bound": "mfma", "peak_tflops": PEAK_TFLOPS["f32"],
                                 "note": "exact fp32 MFMAs: 1e-7 from the reference (tests/test_engine_gpu.py)"},
            "split_parity_mode": {"utt_per_s": round(ups["split"], 3), "batches_in_flight": K2, "kernel": ksp,
                                  "achieved_tflops_algorithmic": round(flsp / (mssp * 1e-3) / 1e12, 1) if mssp > 0 else None,
                                  "note": "DIFFSEP_F32_SPLIT: fp32 tensors, every MFMA product as 3 bf16 MFMAs on hi / lo "
                                          "halves (tests/test_split_gpu.py)"}}
        # parity-grade throughput: the fastest mode inside the 1e-3 absolute RMS bar
        extra_json["_ups"] = {k: v for k, v in ups.items()}
        extra_json["_abs"] = {k: max(absr[k] / 1e-3, rel[k] / 1e-2) for k in absr}  # (inside the bar: < 1)
        for e in e32 + esp + eot:
            e.close()
        if args.nf != 128 and not args.no_nf128:
            # ---- the published model width (icassp-separation.yaml:14-18, nr.yaml): nf = 128 in the main dtype
            # (spec_factor 0.15 as published — icassp-separation.yaml:17 — not the 0.33 of the nf = 64 default: the smaller
            # spectrogram scale is what makes 16-bit rounding cost more at this width, tests/test_fullsize_gpu.py)
            SF128 = 0.15
            cfg128 = _lib.model_config(nf=128, num_sources=S, dtype=dt_flag, spec_factor=SF128)
            sd128 = synth.synth_state_dict([(n, s_) for n, s_, _ in param_table(cfg128)], 7)
            blob128 = pack_state_dict(cfg128, sd128)
            e128 = [Engine(cfg128, blob128) for _ in range(K2)]
            u128 = time_mode(e128, 4)
            sync()
            t3 = time.perf_counter()
            run_on(e128, 77, 0)
            sync()
            alone128 = (time.perf_counter() - t3) * 1e3
            k128, (n128, ms128, fl128) = dominant(e128)
            extra_json["nf128"] = {"utt_per_s": round(u128, 3), "batches_in_flight": K2, "one_batch_alone_ms": round(alone128, 1),
                                   "realtime_factor": round(u128 * T / 8000.0, 1), "dtype": args.dtype, "spec_factor": SF128,
                                   "dominant_kernel": k128, "launches": n128, "avg_launch_us": round(ms128 / n128 * 1e3, 1),
                                   "frac_mfma": round(fl128 / (ms128 * 1e-3) / 1e12 / PEAK_TFLOPS[args.dtype], 4),
                                   "model_tflops": round(u128 * nfe * GFLOP_PER_NFE[128] * (T / 32000.0) / 1e3, 1)}
            if args.dtype == "f16":
                # what dtype="auto" SHIPS at this width (pl_model: hybrid for nf > 64): a split engine for the first
                # HYBRID_HEAD_STEPS reverse steps, the f16 engine after — throughput on the same clock and the agreement of
                # both modes with the exact fp32 engine on the same noise
                from diffsep_amd.pl_model import HYBRID_HEAD_STEPS
                h128 = [Engine(_lib.model_config(nf=128, num_sources=S, dtype=_lib.F32_SPLIT, spec_factor=SF128), blob128, lib_kind="f16") for _ in range(K2)]

                def run_h128(i, w):
                    with on_stream(w):
                        mn, _, _ = ops.normalize_batch(mix)
                        sep, _ = e128[w].pc_sample(mn, sde, N=args.N, corrector_steps=args.corrector_steps, snr=0.5, eps=0.03,
                                                   denoise=True, seed=2000 + i, tail=h128[w], head_steps=HYBRID_HEAD_STEPS)
                        out = ops.scale_output(mix, sep)
                    keep[w] = (mn, sep, out)
                for w in range(K2):
                    run_h128(w, w); run_h128(w, w)
                sync()
                t5 = time.perf_counter()
                for i in range(4):
                    run_h128(i, i % K2)
                sync()
                uh128 = B * 4 / (time.perf_counter() - t5)
                f128 = Engine(_lib.model_config(nf=128, num_sources=S, dtype=_lib.F32, spec_factor=SF128), blob128)
                Bq = min(B, 4)  # (the exact fp32 engine at this width: a few utterances are enough for the agreement figures)
                mq, mnq = mix[:Bq].contiguous(), mix_norm0[:Bq].contiguous()
                r32 = ops.scale_output(mq, f128.pc_sample(mnq, sde, **kw)[0])
                rh = ops.scale_output(mq, e128[0].pc_sample(mnq, sde, tail=h128[0], head_steps=HYBRID_HEAD_STEPS, **kw)[0])
                r16 = ops.scale_output(mq, e128[0].pc_sample(mnq, sde, **kw)[0])

                def qual(v):
                    q_ = si_sdr_db(v, r32)
                    return {"si_sdr_db_vs_fp32": round(float(q_.mean()), 2), "si_sdr_db_vs_fp32_min": round(float(q_.min()), 2),
                            "rel_rms_vs_fp32": float("%.3e" % float(((v - r32).double().pow(2).mean() / r32.double().pow(2).mean()).sqrt())),
                            "abs_rms_vs_fp32": float("%.3e" % float((v - r32).double().pow(2).mean().sqrt()))}
                extra_json["nf128"]["hybrid"] = {"utt_per_s": round(uh128, 3), "batches_in_flight": K2, "head_steps": HYBRID_HEAD_STEPS,
                                                 "realtime_factor": round(uh128 * T / 8000.0, 1), **qual(rh),
                                                 "note": "the mode dtype='auto' ships at nf > 64 (pl_model.DiffSepModel); agreement on %d utterances" % Bq}
                extra_json["nf128"]["f16_quality"] = qual(r16)
                f128.close()
                for e in h128:
                    e.close()
            for e in e128:
                e.close()

    ranks_seen = [0]
    rank_elapsed = [elapsed]
    rank_mem = [[K, int(per_engine), int(hbm_free)]]
    if world > 1:
        # every rank's own time over the timed region (the job's time is the slowest rank's) and memory situation
        tt = torch.tensor([elapsed, float(K), float(per_engine), float(hbm_free)], dtype=torch.float64, device=dev)
        parts = [torch.zeros_like(tt) for _ in range(world)]
        dist.all_gather(parts, tt)
        rank_elapsed = [float(q[0]) for q in parts]
        rank_mem = [[int(q[1]), int(q[2]), int(q[3])] for q in parts]
        elapsed = max(rank_elapsed)
        ranks_seen = seen_ranks(dist, world, rank, local_rank, dev)

    if rank == 0:
        utt = B * world * args.steps
        value = utt / elapsed
        res = {
            "metric": "separated utterances/sec (4 s, 8 kHz, 2-spk, N=30 PC steps)",
            "value": round(value, 4), "unit": "utterances/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 2), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "configs[1]: 2-spk N=%d PC sampler (+%d ald2 corrector step), batch=%d x %.1f s @ 8 kHz "
                                   "per GPU and step, NCSN++ nf=%d random-init, %d NFE/step; %d consecutive steps (batches) in "
                                   "flight per GPU" % (args.N, args.corrector_steps, B, T / 8000.0, args.nf, nfe, K),
                       "batch_per_gpu": B, "samples": T, "N": args.N, "corrector_steps": args.corrector_steps,
                       "nf": args.nf, "sharding": "utterances/%d" % world, "graph": not args.no_graph,
                       "batches_in_flight": K},
            "realtime_factor": round(value * T / 8000.0, 2),
            "nfe_per_s": round(value * nfe, 1),
            "model_tflops": round(value * nfe * GFLOP_PER_NFE.get(args.nf, float("nan")) * (T / 32000.0) / 1e3, 2),
            "finite": finite,
            "device_bytes": sum(e.device_bytes() for e in engs),
            "ranks_seen": ranks_seen,  # [rank, local device] of every rank that took part (all-gather)
            # weak scaling: every rank does the same work, so max / mean of the ranks' own times is the imbalance the
            # slowest GPU (clocks, neighbours on the fabric) imposes on the job
            "rank_elapsed_s_per_step": [round(t_ / args.steps, 4) for t_ in rank_elapsed],
            "imbalance_max_over_mean": round(max(rank_elapsed) / (sum(rank_elapsed) / len(rank_elapsed)), 4),
            "hbm": {"engines_per_rank": [m_[0] for m_ in rank_mem], "bytes_per_engine": rank_mem[0][1],
                    "free_bytes_before_engines_min": min(m_[2] for m_ in rank_mem),
                    "note": "one process and one set of engines per GPU; GPU_MAX_HW_QUEUES=8 is per process (its own device), "
                            "so eight ranks do not share hardware queues"},
        }
        if alone_ms is not None:
            res["config"]["one_batch_alone_ms"] = round(alone_ms, 2)
            res.update({
                "one_batch_alone_ms": round(alone_ms, 2),
                "throughput_mode": ({"rw_quarter": True, "one_batch_alone_ms_in_this_mode": round(alone_spread_ms, 2),
                                     "note": "timed region: register-weight launches with <= 4 tiles per block on a quarter of the CUs (engine option "
                                             "rw_quarter, set by multi-stream callers); one_batch_alone_ms and roofline: the engine's default "
                                             "configuration (every launch on all CUs), measured after the timed region on engine 0"}
                                    if alone_spread_ms is not None else None),
                "utt_per_s_per_gpu_one_batch_at_a_time": round(B / (alone_ms * 1e-3), 2),
                "in_flight_bit_identical": same_bits})
        if roof is not None:
            res["roofline"] = roof
        ups_ = extra_json.pop("_ups", None)
        abs_ = extra_json.pop("_abs", None)
        if ups_ is not None:
            # parity-grade throughput: the fastest of the measured modes whose output is inside 1e-3 absolute and 1 %
            # relative RMS of the exact fp32 engine's
            cand = {args.dtype: value, **ups_}
            ok = {k: v for k, v in cand.items() if k == "f32" or abs_.get(k, 9.0) < 1.0}
            best = max(ok, key=lambda k: ok[k])
            res["value_parity_grade"] = round(ok[best], 4)
            res["parity_grade_mode"] = best
        res.update(extra_json)
        # BASELINE.json configs[1] says bf16 literally; `value` is the shipped default (f16: the same kernels and tensor width on IEEE
        # half precision, the finer significand).  The literal-config number is reported at top level too.
        res["config_dtype_literal"] = "bf16"
        if args.dtype == "bf16":
            res["value_bf16"] = res["value"]
        elif "bf16_mode" in res:
            res["value_bf16"] = res["bf16_mode"]["utt_per_s"]
        if args.full and not args.no_cpu_baseline and world == 1 and not dry:
            t_utt, n_cpu, t_nfe, cores = cpu_baseline(args.nf, T, args.N, args.corrector_steps)
            res["cpu_baseline"] = {"value": round(1.0 / t_utt, 5), "unit": "utterances/s", "cores": cores, "kind": "port",
                                   "sample_kind": "full_run",
                                   "sample": "ONE utterance (B=1, T=%d) end to end through the fp32 torch-CPU oracle: normalize_batch, the "
                                             "full PC sampler (N=%d, %d corrector step: %d network evaluations STFT->NCSN++ nf=%d->iSTFT "
                                             "on injected noise), scale_output: %.2f s (one evaluation alone: %.3f s)"
                                             % (T, args.N, args.corrector_steps, n_cpu, args.nf, t_utt, t_nfe)}
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
