"""Cost of the device LLR / WSS / segmental SNR (diffsep_composite, csrc/composite.hip) on one GPU, beside the host form.

    python tools/composite_bench.py [--reps 50] [--warmup 5] [--host-threads 16] [--no-host]

One batch: B = 16, S = 1, T = 160000, fs = 16000 (16 files of 10 s, 1329 frames each: what evaluate_covl --batch 16 hands
over).  Device: the whole launch sequence of one ops.composite call between two HIP events on the current stream, median / min /
max of --reps calls after --warmup calls, clocks as found.  Host: wall time of diffsep_amd.metrics.composite over the same files
on --host-threads threads, median of 3, and the single-thread cost per file.  Prints one JSON line.  For the per-kernel split run
it once under `rocprofv3 --kernel-trace --stats -- python tools/composite_bench.py --no-host --reps 20`.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-separation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffsep_amd import metrics, ops, synth  # noqa: E402

CASE = dict(B=16, S=1, T=160000, fs=16000)


def inputs(B, S, T, fs):
    ref = np.stack([synth.synth_mixture(i, T=T, fs=fs, n_src=max(S, 2))[1][:S] for i in range(B)]).astype(np.float32)
    est = np.stack([[r + 0.3 * np.std(r) * synth.normal(f"bench{s}", T, i) for s, r in enumerate(ref[i])]
                    for i in range(B)]).astype(np.float32)
    return ref, est


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    B, S, T, fs = CASE["B"], CASE["S"], CASE["T"], CASE["fs"]
    ref, est = inputs(B, S, T, fs)
    ref_d, est_d = torch.from_numpy(ref).cuda(), torch.from_numpy(est).cuda()
    for _ in range(args.warmup):
        out = ops.composite(ref_d, est_d, fs)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = ops.composite(ref_d, est_d, fs)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    got = out.cpu().numpy()
    res = dict(CASE, files=B * S, frames_per_file=int(got[0, 0, 3]), reps=args.reps, device_ms_median=round(median(ms), 4),
               device_ms_min=round(min(ms), 4), device_ms_max=round(max(ms), 4),
               workspace_MB=round(ops.composite_workspace_bytes(B, S, T, fs) / 2 ** 20, 2),
               mean_llr=round(float(got[..., 0].mean()), 6), mean_wss=round(float(got[..., 1].mean()), 6),
               mean_segsnr=round(float(got[..., 2].mean()), 6))
    if not args.no_host:
        jobs = [(ref[b, s], est[b, s]) for b in range(B) for s in range(S)]
        ones = []
        for j in jobs[:4]:  # (the first call builds the filter bank: not counted)
            t0 = time.perf_counter()
            metrics.composite(j[0], j[1], fs)
            ones.append(time.perf_counter() - t0)
        walls = []
        with ThreadPoolExecutor(max_workers=args.host_threads) as pool:
            for _ in range(3):
                t0 = time.perf_counter()
                vals = list(pool.map(lambda j: metrics.composite(j[0], j[1], fs), jobs))
                walls.append(time.perf_counter() - t0)
        host = np.array([[v["llr"], v["wss"], v["segsnr"]] for v in vals]).reshape(B, S, 3)
        res.update(host_threads=args.host_threads, host_wall_ms_median=round(median(walls) * 1e3, 2),
                   host_wall_ms_all=[round(w * 1e3, 2) for w in walls], host_ms_per_file_one_thread=round(median(ones[1:]) * 1e3, 2),
                   max_abs_diff=float(np.max(np.abs(got[..., :3] - host))))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
